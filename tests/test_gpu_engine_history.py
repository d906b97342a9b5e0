"""An engine's history never changes an enqueue's bits ("Engine history"); run with -m gpu on an MI355X.

ONE engine is driven through sequences of steps (tests/engine_history.py: settings, a pair list, optional initial states)
and after every step its result -- states, every field of every phovo_pair_report, the trust-region records or
(alpha, beta), the launch records -- must be, bit for bit, what a fresh engine gives for that step alone.  What the
sequences cross is the host code of phovo_engine_enqueue_align and phovo_engine_evaluate_pairs that lets kernels share
scratch from one enqueue to the next: the per-slot owner buffer and its `owner_tagged` flag, its hand-over between the
two slots, the pair data and its pinned mirror, the work-queue heads and hand-over lists, d_tr_reports, d_illum, the wide
form's workspace, the evaluate workspace and its watermark.

Fresh results are cached per distinct step and each is held once to its CPU checker (bit equality alone would also hold
if both were wrong).  Every step's launch kinds are literal data and asserted; the transitions a sequence must contain
are derived from the launch records OBSERVED, not from the steps' labels.
"""
import ctypes as C

import numpy as np
import pytest

import engine_history as eh

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------------
class Driver:
    """One engine and what this caller last set on it.  A setter is called only when its value changes (set_config waits
    for every enqueue in flight: calling it needlessly would serialise the pipelined stretches).  Which changes drop the
    frame pool the driver does not know: it learns it from PHOVO_E_NOT_READY at the align, re-reserves, uploads, and
    repeats the call (phovo_hip.h)."""

    def __init__(self):
        self.eng = odometry.AlignmentEngine()
        self.eng.set_build_all_levels(True)          # the pool's layout stays put when a configuration skips a level
        self.eng.set_trust_region_options(eh.trust_region_options())
        self.applied = {}
        self.pool = None
        self.uploads = 0
        self._config((4, 4), (0.0, 0.0))

    def close(self):
        self.eng.close()

    def _apply(self, key, value, setter):
        if self.applied.get(key) != value:
            setter()
            self.applied[key] = value

    def _config(self, max_iter, min_grad):
        cfg = native.make_config(num_levels=eh.NUM_LEVELS, max_iter=list(max_iter), min_grad=list(min_grad))
        self._apply("config", (max_iter, min_grad), lambda: self.eng.set_config(cfg))

    def _objective_and_extensions(self, objective, bilinear, huber):
        def ext():
            sampling = native.SAMPLING_BILINEAR if bilinear else native.SAMPLING_NEAREST_SCATTER
            self._apply("ext", (bilinear, tuple(huber or ())),
                        lambda: self.eng.set_extensions(native.make_extensions(huber_delta=huber, sampling=sampling)))

        def obj():
            self._apply("objective", objective, lambda: self.eng.set_objective(eh.OBJECTIVES[objective]))
        # (the setter that comes second refuses a combination the objective does not support)
        for f in ((obj, ext) if objective == "photometric" else (ext, obj)):
            f()

    def configure(self, step):
        e = self.eng
        self._objective_and_extensions(step.objective, step.bilinear, eh.huber_deltas(step))
        self._config(step.max_iter, step.min_grad)
        self._apply("wide", step.wide_policy, lambda: e.set_wide_policy(step.wide_policy))
        self._apply("slide", step.slide_policy, lambda: e.set_slide_policy(step.slide_policy))
        self._apply("fusion", step.fusion, lambda: e.set_level_fusion(step.fusion))
        self._apply("latency", step.latency, lambda: e.set_latency_forms(step.latency))
        self._apply("invariant", step.batch_invariant, lambda: e.set_batch_invariant(step.batch_invariant))
        if step.pool != self.pool:
            self.upload(step.pool)

    def upload(self, pool):
        probs = eh.pool_problems(pool)
        w, h = eh.POOLS[pool]
        self.eng.set_intrinsic_matrix(probs[0]["K"])
        self.eng.reserve_frames(2 * len(probs), w, h)
        for c, p in enumerate(probs):
            self.eng.upload_frame(2 * c, p["gray0"], p["depth0"])
            self.eng.upload_frame(2 * c + 1, p["gray1"], p["depth1"])
        self.pool = pool
        self.uploads += 1

    def _retry_after_upload(self, pool, call):
        try:
            return call()
        except native.PhovoError as err:
            if err.status != native.E_NOT_READY:
                raise
        self.upload(pool)                            # a settings change dropped the pool
        return call()

    def level_pixels(self):
        return {l: int(np.prod(self.eng.level_size(l))) for l in range(eh.NUM_LEVELS)}

    def enqueue(self, step):
        """Issues the step; returns what finish() needs.  The launch records, the trust-region records and (alpha, beta)
        speak of the LAST enqueue, so they are read before the next one is issued (the latter two wait for this enqueue's
        stream only)."""
        self.configure(step)
        src, tgt, init = eh.pair_list(step)
        n = self._retry_after_upload(step.pool, lambda: self.eng.enqueue_align(src, tgt, init))
        out = dict(step=step, n=n, ticket=self.eng.last_ticket(), records=self.eng.last_launches(), tr=None, illum=None,
                   level_pixels=self.level_pixels())
        if step.objective == "trust_region":
            out["tr"] = self.eng.trust_region_reports(n)
        if step.objective == "affine":
            out["illum"] = self.eng.fetch_illumination(n)
        return out

    def finish(self, pending):
        states, reps = self.eng.fetch(pending["ticket"], pending["n"], want_reports=True)
        pending.update(states=states, reports=reps, report_bytes=b"".join(bytes(memoryview(r)) for r in reps),
                       launches=[(r["kind"], tuple(r["levels"]), r["threads"], r["lds_bytes"], r["workgroups"])
                                 for r in pending["records"]])
        return pending

    def align(self, step):
        return self.finish(self.enqueue(step))

    def evaluate(self, call):
        pool = self.pool or "A"
        self._objective_and_extensions("photometric", False, None)
        src, tgt, states, level = eh.eval_arguments(pool, call)
        res = self._retry_after_upload(pool, lambda: self.eng.evaluate_pairs(src, tgt, states, level, want_structs=True))
        res["struct_bytes"] = b"".join(bytes(memoryview(s)) for s in res.pop("structs"))
        return pool, res


def first_difference(got, want):
    """The first field in which two results of a step differ, or None."""
    if got["launches"] != want["launches"]:
        return f"launch records: {got['launches']} != {want['launches']}"
    if not np.array_equal(got["states"], want["states"], equal_nan=True):
        k = int(np.argmax([not np.array_equal(a, b, equal_nan=True) for a, b in zip(got["states"], want["states"])]))
        return f"states[{k}]: {got['states'][k]} != {want['states'][k]}"
    if got["report_bytes"] != want["report_bytes"]:
        for k, (a, b) in enumerate(zip(got["reports"], want["reports"])):
            if bytes(memoryview(a)) == bytes(memoryview(b)):
                continue
            for name, _ in native.PairReport._fields_:
                x, y = getattr(a, name), getattr(b, name)
                x, y = (list(x), list(y)) if isinstance(x, C.Array) else (x, y)
                if not np.array_equal(x, y, equal_nan=True):
                    return f"reports[{k}].{name}: {x} != {y}"
            return f"reports[{k}]: bytes that belong to no field"
    for what in ("tr", "illum"):
        a, b = got[what], want[what]
        if (a is None) != (b is None):
            return f"{what}: present on one side only"
        if a is None:
            continue
        for name in (a.dtype.names or [None]):
            x, y = (a, b) if name is None else (a[name], b[name])
            if not np.array_equal(x, y, equal_nan=True):
                k = int(np.argmax([not np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y)]))
                return f"{what}{'' if name is None else '.' + name}[{k}]: {x[k]} != {y[k]}"
    return None


def first_eval_difference(got, want):
    for name in ("information", "gradient", "cost", "rows", "flags"):
        if not np.array_equal(got[name], want[name], equal_nan=True):
            k = int(np.argmax([not np.array_equal(p, q, equal_nan=True) for p, q in zip(got[name], want[name])]))
            return f"{name}[{k}]: {got[name][k]} != {want[name][k]}"
    return None if got["struct_bytes"] == want["struct_bytes"] else "struct bytes"


# ------------------------------------------------------------------------------------------------------------------------
# fresh results: one new engine per distinct step (and per distinct evaluate call), cached for the whole module
# ------------------------------------------------------------------------------------------------------------------------
_fresh, _fresh_eval = {}, {}


def fresh(step):
    if step.name not in _fresh:
        d = Driver()
        try:
            _fresh[step.name] = d.align(step)
        finally:
            d.close()
    return _fresh[step.name]


def fresh_eval(pool, call):
    if (pool, call) not in _fresh_eval:
        d = Driver()
        try:
            d.upload(pool)
            _fresh_eval[pool, call] = d.evaluate(call)[1]
        finally:
            d.close()
    return _fresh_eval[pool, call]


def run_sequence(sequence, label):
    """Drives one engine through the sequence; after every step, the bytes of its fresh result.  Returns one record per
    enqueue, in ticket order: (step, user OBSERVED from the launch records, pairs, launch kinds)."""
    history, observed = [], []

    def fail(what, difference):
        before = "\n    ".join(history[-5:-1])
        raise AssertionError(f"{label}: item {len(history) - 1} differs from the same on a fresh engine\n  at: {what}\n"
                             f"  first difference: {difference}\n  the four items before it:\n    {before}")

    def check_step(res):
        step = res["step"]
        observed.append((step, eh.classify(res["records"], res["level_pixels"]), res["n"], tuple(r[0] for r in res["launches"])))
        assert observed[-1][3] == step.kinds, (label, len(history) - 1, str(step), observed[-1][3])
        diff = first_difference(res, fresh(step))
        if diff:
            fail(str(step), diff)

    def check_eval(d, call):
        pool, res = d.evaluate(call)
        diff = first_eval_difference(res, fresh_eval(pool, call))
        if diff:
            fail(f"evaluate call {call} {eh.EVAL_CALLS[call]} on pool {pool}", diff)

    d = Driver()
    try:
        for kind, what in sequence:
            if kind == "align":
                history.append(f"align {eh.VOCABULARY[what]}")
                check_step(d.align(eh.VOCABULARY[what]))
            elif kind == "eval":
                history.append(f"evaluate call {what} {eh.EVAL_CALLS[what]}")
                check_eval(d, what)
            else:
                pending = None
                for name in what:
                    if name.startswith("eval:"):
                        history.append(f"evaluate call {name[5:]} (behind an enqueue not yet fetched)")
                        check_eval(d, int(name[5:]))
                        continue
                    history.append(f"enqueue {eh.VOCABULARY[name]} (pipelined)")
                    issued = d.enqueue(eh.VOCABULARY[name])
                    if pending:                       # one behind: the other slot's enqueue may still be running
                        check_step(d.finish(pending))
                    pending = issued
                check_step(d.finish(pending))
    finally:
        d.close()
    return observed


# ------------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", sorted(eh.POOLS))
def test_pools_have_one_level_in_lds_and_one_in_hbm(pool):
    """The smallest shapes at which the shared buffer is used at all: level 1 keeps its owner map in LDS, level 0 in HBM,
    under each of the three objectives that have one."""
    for objective in ("photometric", "biobjective", "trust_region"):
        res = fresh({"photometric": eh.VOCABULARY["exact40" if pool == "A" else "B_exact48"],
                     "biobjective": eh.VOCABULARY["bi40" if pool == "A" else "B_bi2"],
                     "trust_region": eh.VOCABULARY["tr40" if pool == "A" else "B_tr40"]}[objective])
        n = res["level_pixels"]
        in_lds = {r["levels"][0]: r["lds_bytes"] >= 4 * n[r["levels"][0]] for r in res["records"]}
        assert in_lds == {1: True, 0: False}, (pool, objective, res["records"])
    d = Driver()
    try:
        d.upload(pool)
        assert d.eng.level_launch_info(1)["owner_in_lds"] and not d.eng.level_launch_info(0)["owner_in_lds"]
    finally:
        d.close()


WORST = {}


@pytest.mark.parametrize("name", list(eh.VOCABULARY))
def test_fresh_result_matches_its_checker(name):
    """Every distinct step, alone on a new engine: the launch kinds it is in the list for, the user of the owner buffer
    it is labelled as (from the launch records), and every pair against the CPU checker of its objective by that
    objective's own rules -- iteration counts, row counts and flags exact, the pose within 1e-9 x max(1, cond / 1e5)."""
    step = eh.VOCABULARY[name]
    res = fresh(step)
    assert tuple(r[0] for r in res["launches"]) == step.kinds, res["launches"]
    assert eh.classify(res["records"], res["level_pixels"]) == step.user, res["records"]
    if len(step.which) >= 512:
        assert any(r["workgroups"] < len(step.which) for r in res["records"])      # a persistent grid drawing from the queues
    worst = 0.0
    for k, case in enumerate(step.which):
        a = eh.anchor(step, case)
        ab = None if res["illum"] is None else res["illum"][k]
        worst = max(worst, a.check(res["states"][k], res["reports"][k], res["tr"], k, ab))
    WORST[name] = worst
    print(f"{name}: worst distance / bar {worst:.2e}; launches {res['launches']}")
    flags = [r.flags for r in res["reports"]]
    if 3 in step.which:
        # the large rotation leaves the window (at once, and drifting out): handed over to the exact kernel
        for k, case in enumerate(step.which):
            assert flags[k] == (native.PAIR_WINDOW_FALLBACK if case >= 3 else 0), (k, case, flags[k])
    else:
        assert not any(flags), flags
    for level in step.skipped:
        assert np.all(res["tr"]["termination"][:, level] == native.TR_SKIPPED) and np.all(res["tr"]["steps"][:, level] == 0)
    if step.objective == "trust_region":
        active = [l for l in range(eh.NUM_LEVELS) if l not in step.skipped]
        assert np.all(res["tr"]["termination"][:, active] != native.TR_SKIPPED)
    if step.min_grad != (0.0, 0.0):
        its = np.array([list(r.iterations[:eh.NUM_LEVELS]) for r in res["reports"][:3]])
        assert np.all(its.min(axis=0) < np.array(step.max_iter)) and len({tuple(i) for i in its}) > 1, its


def _slot_distance_2(observed, first, second):
    """Is there an enqueue of step `first` followed, two enqueues later (the same slot), by one of step `second`?"""
    names = [o[0].name for o in observed]
    return any(a == first and b == second for a, b in zip(names, names[2:]))


def test_scripted_sequence():
    """The serial sequence (align_pairs, one enqueue in flight; consecutive enqueues alternate slots).  From the launch
    records OBSERVED: every tagger -> wide, wide -> every tagger and every ordered pair of different taggers at distance 1
    (the hand-over, or free-both-and-reallocate) and 2 (the slot keeps its buffer); a tagged buffer that sits through two
    non-user enqueues of its slot before a wide step; 40 -> 48 -> 2 -> 520 -> 40 pairs under each objective (owner buffer,
    pair data, d_tr_reports, d_illum), the 520-pair slot then serving 2 and later 520 again; initial states and then none;
    all levels and then a skipped one; pool B and back, from larger and from smaller scratch."""
    observed = run_sequence(eh.SCRIPTED, "scripted sequence")
    users = [o[1] for o in observed]
    missing = eh.required_transitions() - eh.transitions(users)
    assert not missing, sorted(missing)
    assert eh.sits_through_non_users(users) == set(eh.TAGGERS), eh.sits_through_non_users(users)
    sizes = {}
    for step, user, n, kinds in observed:
        sizes.setdefault((frozenset(kinds), step.pool), []).append(n)
    want = [int(g) for g in eh.GROWTH]
    for kinds in (("persistent",), ("biobjective",), ("trust_region",), ("affine",)):
        run = sizes[frozenset(kinds), "A"]
        assert any(run[i:i + len(want)] == want for i in range(len(run))), (kinds, run)
    assert _slot_distance_2(observed, "exact40_init", "exact40")
    assert _slot_distance_2(observed, "tr40", "tr40_skip") and _slot_distance_2(observed, "tr48", "tr40_skip")
    pools = [o[0].pool for o in observed]
    moves = [(observed[i - 1][2], observed[i][2]) for i in range(1, len(pools)) if pools[i - 1] == "A" and pools[i] == "B"]
    assert any(a > b for a, b in moves), moves               # scratch sized for more than pool B's step needs
    back = [(observed[i - 1][2], observed[i][2]) for i in range(1, len(pools)) if pools[i - 1] == "B" and pools[i] == "A"]
    assert any(a < b for a, b in back), back                 # ... and for less than pool A's step needs
    assert any(o[2] >= 512 for o in observed)                # eight work queues, the larger pair layout


def test_two_enqueues_in_flight():
    """enqueue_align / fetch(ticket), one behind, as in the header's loop: the 1040-iteration step (40 pairs, the
    persistent kernel with its owner map in HBM) followed by a short one of every user kind, and short ones followed by
    the long one.  Whether the engine finds the other slot idle depends on timing; both branches are legitimate and
    neither is asserted -- only the fresh bytes, and that both tickets stay fetchable."""
    observed = run_sequence(eh.PIPELINED, "two enqueues in flight")
    users = [o[1] for o in observed]
    after_long = {users[i] for i in range(1, len(users)) if observed[i - 1][0].name == "long40"}
    assert after_long >= set(eh.USERS) | {"none"}, after_long
    before_long = {users[i - 1] for i in range(1, len(users)) if observed[i][0].name == "long40"}
    assert before_long >= {"wide", "tr-HBM"}, before_long


def test_fetch_reports_the_levels_of_its_own_enqueue():
    """Regression (found by the pipelined sequences): phovo_engine_fetch filled in `iterations = 1` for the levels that
    the configuration IN FORCE AT THE FETCH skips.  With a set_config between an enqueue and its fetch -- the next
    enqueue's -- the report lost its own level's count and kept a zero where the reference reports one pass."""
    run_sequence([("pipe", ("exact40", "lds40", "exact40", "tr40_skip", "lds2"))], "fetch after set_config")


def test_evaluate_between_aligns():
    """phovo_engine_evaluate_pairs between aligns and between an enqueue and its fetch: level 1 with 1 pair, level 0 with
    more pairs than one 256 MB group holds, level 1 with 3 pairs, level 0 with 1 pair (the eval_owner_clean watermark goes
    up, is undercut, and is passed on the level whose maps are four times the size).  Every call is the bytes of the same
    call on a fresh engine, and the aligns around it are unchanged.  A second engine grows its workspace while the
    watermark alone would call it clean (four level-1 maps behind one level-0 map)."""
    level, n = eh.EVAL_CALLS[1]
    assert level == 0 and n > eh.eval_group("A", 0) and n > eh.eval_group("B", 0)
    run_sequence(eh.WITH_EVALUATE, "evaluate between aligns")
    run_sequence(eh.EVALUATE_REGROWN, "evaluate, workspace regrown")


@pytest.mark.parametrize("seed", eh.RANDOM_SEEDS)
def test_random_sequence(seed):
    run_sequence(eh.random_sequence(seed, eh.RANDOM_LENGTH), f"random sequence, seed {seed}")
