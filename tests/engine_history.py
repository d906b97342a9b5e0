"""Steps and sequences of tests/test_gpu_engine_history.py (one engine driven through a mixed workload must give, after
every step, the bytes a fresh engine gives for that step alone; DESIGN.md §4, "Engine history"), with what the CPU checkers
say about every step.  tests/test_engine_history_cpu.py holds the vocabulary to the guards the GPU file relies on and
the sequences to the transitions they promise, without a device.  Plain Python, no device; test infrastructure, not
collected.

A STEP is the engine settings that matter, a pair list and optional initial states.  The users of the per-slot owner
buffer in HBM (phovo_engine_enqueue_align):
  wide             the many-workgroups form: needs -1 everywhere and leaves it so
  persistent-HBM   gn_level_kernel with its owner map in HBM            \
  slide+fallback   the sliding-window launch and its exact fall-back      | the taggers: leave tagged entries behind
  bi-HBM           the bi-objective's HBM geometry                       |
  tr-HBM           the trust region's (one map per resident workgroup)  /
  none             affine, bilinear, and steps whose active levels keep their owner maps in LDS
A sequence is a list of items:
  ("align", name)              align_pairs of VOCABULARY[name]
  ("pipe", (name, name, ...))  the same steps through enqueue_align / fetch(ticket), one behind; an entry "eval:<i>" is
                               an evaluate call between an enqueue and its fetch
  ("eval", i)                  EVAL_CALLS[i]
A step names its pool; the driver re-reserves when the pool changes.
"""
import dataclasses
import functools

import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import native, se3, synthetic
from oracle import oracle

import affine_ref as ar
import test_gpu_objective_edges as goe
import test_gpu_trust_region as gtr
import trust_region_ref as tref
from test_gpu_large_rotations import Expect, _cond

NUM_LEVELS = 2
POOLS = {"A": (320, 240), "B": (330, 250)}          # level 1: owner map in LDS; level 0: in HBM
TAGGERS = ("persistent-HBM", "slide+fallback", "bi-HBM", "tr-HBM")
USERS = ("wide",) + TAGGERS
DELTA = 0.05                                         # Huber delta (extension_forms.DELTA)
LONG_ITERATIONS = 1040                               # crosses the owner tags' period of 1023
EVAL_GROUP_BYTES = 256 << 20                         # owner maps of one evaluation group (phovo_hip.h)

# cases of a pair list: 0..2 the pool's three problems from rest, 3 / 4 the large in-plane rotation of
# test_sliding_window_hands_large_motions_to_the_exact_kernel, out of the window at once / drifting out of it (pool A only)
BIG_MOTION = [0.01, -0.005, 0.004, 0.30, 0.002, -0.003]
BIG_NEAR = np.array([0.004, 0.002, -0.003, 0.004, -0.002, 0.001])
BIG_DRIFT = np.array([0.0, 0.0, 0.0, 0.17, 0.0, 0.0])
# non-zero initial states of cases 0..2 (steps with inits=True)
INITS = np.array([[0.004, -0.003, 0.002, 0.0015, -0.001, 0.002],
                  [-0.005, 0.002, 0.003, -0.002, 0.0015, -0.001],
                  [0.003, 0.004, -0.002, 0.001, 0.002, -0.0015]])


@functools.lru_cache(maxsize=None)
def pool_problems(pool):
    """The frame pairs of a pool: frame 2c is problem c's source, 2c + 1 its target (both with depth: the bi-objective)."""
    w, h = POOLS[pool]
    probs = [synthetic.make_pair(80 + i, w, h, holes=0.02 * i, trans=0.01 * (i + 1), rot=0.004 * (i + 1)) for i in range(3)]
    if pool == "A":
        probs.append(synthetic.render_pair_with_motion(91, w, h, BIG_MOTION))
    return probs


def case_problem(case):
    return min(case, 3)


def case_init(pool, case, inits):
    if case == 3:
        return pool_problems(pool)[3]["motion"] + BIG_NEAR
    if case == 4:
        return BIG_DRIFT.copy()
    return INITS[case].copy() if inits else np.zeros(6)


@dataclasses.dataclass(frozen=True)
class Step:
    name: str
    user: str                            # what the step is in the list FOR; the GPU test classifies what it OBSERVED
    kinds: tuple                         # expected launch kinds, in launch order (coarse to fine)
    which: tuple                         # the case of every pair
    pool: str = "A"
    objective: str = "photometric"       # photometric | biobjective | trust_region | affine
    bilinear: bool = False
    huber: bool = False
    wide_policy: int = 0
    slide_policy: int = 0
    fusion: int = native.FUSION_AUTO
    latency: bool = False
    batch_invariant: bool = False
    max_iter: tuple = (4, 4)             # [level 0, level 1]
    min_grad: tuple = (0.0, 0.0)
    inits: bool = False
    skipped: tuple = ()                  # trust region: levels whose records must read TR_SKIPPED

    def __str__(self):
        diff = {f.name: getattr(self, f.name) for f in dataclasses.fields(self)
                if f.name not in ("name", "which", "kinds") and getattr(self, f.name) != f.default}
        return f"{self.name}[{len(self.which)} pairs, {diff}]"


def cycle(n, cases=(0, 1, 2)):
    return tuple(cases[k % len(cases)] for k in range(n))


OBJECTIVES = {"photometric": native.OBJECTIVE_PHOTOMETRIC, "biobjective": native.OBJECTIVE_BIOBJECTIVE,
              "trust_region": native.OBJECTIVE_TRUST_REGION, "affine": native.OBJECTIVE_PHOTOMETRIC_AFFINE}
LDS, PHBM = ("persistent", "persistent"), ("persistent", "persistent")
SLIDE = ("persistent", "slide", "slide_fallback")
THRESHOLDS = (100.0, 200.0)                  # min_gradient_norm of the thresholded configuration (test_engine_history_cpu
#                                          asserts that cases stop by it on both levels and that none is near it)


def _steps():
    P, B, T, A = "photometric", "biobjective", "trust_region", "affine"
    s = [
        # ---- wide ---------------------------------------------------------------------------------------------------
        Step("wide2", "wide", ("persistent", "wide"), cycle(2)),
        Step("wide2_b", "wide", ("persistent", "wide"), cycle(2, (2, 1))),
        Step("wide8_forced", "wide", ("wide", "wide"), cycle(8), wide_policy=1),
        Step("latency1", "wide", ("wide", "wide"), (1,), latency=True),
        Step("latency8", "wide", ("wide", "wide"), cycle(8), latency=True),
        # ---- persistent kernel, owner map in HBM -------------------------------------------------------------------------
        Step("huber2", "persistent-HBM", PHBM, cycle(2), huber=True, slide_policy=-1),
        Step("exact40", "persistent-HBM", PHBM, cycle(40), slide_policy=-1),
        Step("exact40_init", "persistent-HBM", PHBM, cycle(40), slide_policy=-1, inits=True),
        Step("exact48", "persistent-HBM", PHBM, cycle(48), slide_policy=-1),
        Step("exact520", "persistent-HBM", PHBM, cycle(520), slide_policy=-1),
        Step("exact2", "persistent-HBM", PHBM, cycle(2), slide_policy=-1, wide_policy=-1),
        Step("exact2_invariant", "persistent-HBM", PHBM, cycle(2), slide_policy=-1, batch_invariant=True),
        Step("threshold40", "persistent-HBM", PHBM, cycle(40), slide_policy=-1, max_iter=(6, 6), min_grad=THRESHOLDS,
             fusion=native.FUSION_OFF),
        # ---- sliding window + exact fall-back ------------------------------------------------------------------------------
        Step("slide48_handover", "slide+fallback", SLIDE, cycle(48, (0, 3, 4)), max_iter=(6, 4)),
        Step("slide40", "slide+fallback", SLIDE, cycle(40)),
        Step("slide520", "slide+fallback", SLIDE, cycle(520)),
        # ---- bi-objective ------------------------------------------------------------------------------------------------
        Step("bi40", "bi-HBM", ("biobjective",) * 2, cycle(40), objective=B, max_iter=(3, 3)),
        Step("bi48", "bi-HBM", ("biobjective",) * 2, cycle(48), objective=B, max_iter=(3, 3)),
        Step("bi2", "bi-HBM", ("biobjective",) * 2, cycle(2), objective=B, max_iter=(3, 3)),
        Step("bi520", "bi-HBM", ("biobjective",) * 2, cycle(520), objective=B, max_iter=(3, 3)),
        # ---- trust region (from INITS: at the zero state every sample sits on a pixel centre, where the bilinear samples'
        # derivative jumps, and one ulp of fx moves the checker's own result by 1e-7 -- the guard of test_engine_history_cpu) ----
        Step("tr40", "tr-HBM", ("trust_region",) * 2, cycle(40), objective=T, inits=True),
        Step("tr48", "tr-HBM", ("trust_region",) * 2, cycle(48), objective=T, inits=True),
        Step("tr2", "tr-HBM", ("trust_region",) * 2, cycle(2), objective=T, inits=True),
        Step("tr520", "tr-HBM", ("trust_region",) * 2, cycle(520), objective=T, inits=True),
        Step("tr40_skip", "tr-HBM", ("trust_region",), cycle(40), objective=T, inits=True, max_iter=(4, 0), skipped=(1,)),
        # ---- no user of the owner buffer -----------------------------------------------------------------------------------
        Step("affine40", "none", ("affine",) * 2, cycle(40), objective=A, max_iter=(3, 3)),
        Step("affine48", "none", ("affine",) * 2, cycle(48), objective=A, max_iter=(3, 3)),
        Step("affine2", "none", ("affine",) * 2, cycle(2), objective=A, max_iter=(3, 3)),
        Step("affine520", "none", ("affine",) * 2, cycle(520), objective=A, max_iter=(3, 3)),
        Step("bilinear8", "none", ("bilinear",) * 2, cycle(8), bilinear=True, latency=True),
        Step("lds40", "none", ("persistent",), cycle(40), max_iter=(0, 4)),
        Step("lds2", "none", ("persistent",), cycle(2), max_iter=(0, 4)),
        # ---- pool B (330x250) -----------------------------------------------------------------------------------------------
        Step("B_wide2", "wide", ("persistent", "wide"), cycle(2), pool="B"),
        Step("B_slide40", "slide+fallback", SLIDE, cycle(40), pool="B"),
        Step("B_exact48", "persistent-HBM", PHBM, cycle(48), pool="B", slide_policy=-1),
        Step("B_tr40", "tr-HBM", ("trust_region",) * 2, cycle(40), pool="B", objective=T, inits=True),
        Step("B_bi2", "bi-HBM", ("biobjective",) * 2, cycle(2), pool="B", objective=B, max_iter=(3, 3)),
        # ---- the pipelined stretches: one configuration (level 0 only), so that no setter waits between the enqueues --------
        Step("long40", "persistent-HBM", ("persistent",), (0,) * 40, slide_policy=-1, max_iter=(LONG_ITERATIONS, 0)),
        Step("long_wide2", "wide", ("wide",), (0,) * 2, slide_policy=-1, max_iter=(LONG_ITERATIONS, 0)),
        Step("long_tr2", "tr-HBM", ("trust_region",), (0,) * 2, objective=T, inits=True, max_iter=(LONG_ITERATIONS, 0),
             skipped=(1,)),
    ]
    return {x.name: x for x in s}


VOCABULARY = _steps()
# steps a random sequence draws from (the 1040-iteration step only in its own test: it costs a hundred times the others)
DRAWN = tuple(n for n in VOCABULARY if not n.startswith("long"))


# ------------------------------------------------------------------------------------------------------------------------
# what a step hands to the engine
# ------------------------------------------------------------------------------------------------------------------------
def native_config(step):
    return native.make_config(num_levels=NUM_LEVELS, max_iter=list(step.max_iter), min_grad=list(step.min_grad))


def oracle_config(step):
    return oracle.make_config(num_levels=NUM_LEVELS, max_iter=list(step.max_iter), min_grad=list(step.min_grad))


def huber_deltas(step):
    return [DELTA if m > 0 else 0.0 for m in step.max_iter] if step.huber else None


def extensions(step):
    return native.make_extensions(huber_delta=huber_deltas(step),
                                  sampling=native.SAMPLING_BILINEAR if step.bilinear else native.SAMPLING_NEAREST_SCATTER)


def trust_region_options():
    """Ceres's defaults on every level."""
    return native.make_trust_region_options()


def pair_list(step):
    """(src, tgt, init_states or None) of a step."""
    src = [2 * case_problem(c) for c in step.which]
    tgt = [2 * case_problem(c) + 1 for c in step.which]
    if not step.inits and all(c < 3 for c in step.which):
        return src, tgt, None
    return src, tgt, np.stack([case_init(step.pool, c, step.inits) for c in step.which])


# ------------------------------------------------------------------------------------------------------------------------
# evaluate calls: (level, pairs).  One 256 MB group holds 873 pairs of pool A's level 0, so the second call runs in two
# groups and leaves the watermark at a full group; the third needs less than is clean, the fourth less again on the level
# whose maps are four times the size.  The fifth is for a workspace that has only seen the fourth: four level-1 maps are
# exactly one level-0 map, so nothing more has to be clean, but the results of four pairs need a larger workspace -- a
# reallocation at which the watermark alone would say "clean".
# ------------------------------------------------------------------------------------------------------------------------
EVAL_CALLS = ((1, 1), (0, 900), (1, 3), (0, 1), (1, 4))


def eval_arguments(pool, call):
    """(src, tgt, states, level) of EVAL_CALLS[call] on a pool: the three problems in turn, at INITS."""
    level, n = EVAL_CALLS[call]
    which = cycle(n)
    return [2 * c for c in which], [2 * c + 1 for c in which], np.stack([INITS[c] for c in which]), level


def eval_group(pool, level):
    w, h = POOLS[pool]
    lw, lh = oracle.level_size(w, h, level)
    return EVAL_GROUP_BYTES // (4 * lw * lh)


# ------------------------------------------------------------------------------------------------------------------------
# sequences
# ------------------------------------------------------------------------------------------------------------------------
def _al(*names):
    return [("align", n) for n in names]


# Every ordered pair of different users at distance 1 and at distance 2 (W wide, P persistent-HBM, S slide+fallback,
# B bi-HBM, T tr-HBM): a walk over the five that test_engine_history_cpu checks, with each letter's steps taken in turn so
# that batch sizes (and with them capacities: hand-over, keep, free-both-and-reallocate) change along it.
_WALK = "TPWSPBTWBSTPSWTBPSBWPTS"
TRANSITION_WALK = _WALK + _WALK[::-1]          # (the reverse covers every ordered pair again, with other batch sizes)
WALK_STEPS = {"W": ("wide2", "wide2_b", "wide8_forced"), "P": ("exact40", "huber2", "exact48"),
              "S": ("slide48_handover", "slide40"), "B": ("bi40", "bi2", "bi48"), "T": ("tr40", "tr48", "tr2")}


def _walk():
    seen = {k: 0 for k in WALK_STEPS}
    out = []
    for letter in TRANSITION_WALK:
        names = WALK_STEPS[letter]
        out.append(names[seen[letter] % len(names)])
        seen[letter] += 1
    return _al(*out)


# ... and after the 520 pairs their slot serves 2 pairs, and later 520 again
GROWTH = ("40", "48", "2", "520", "40", "2", "40", "520")


def _growth(prefix):
    """40 -> 48 -> 2 -> 520 -> 40 under one objective: every per-slot buffer grows, shrinks and is reused."""
    return _al(*[prefix + n for n in GROWTH])


SCRIPTED = (
    _al("wide2", "exact40", "wide2")
    + _walk()
    # a tagged buffer sits through two non-user enqueues of its own slot before a wide step takes it: tagger on slot s,
    # then (other slot, s, other slot, s) non-users, then wide at distance 6 on slot s; and the same from the other slot
    # (seven steps each, so the four start on alternating slots)
    + _al("exact48", "affine2", "lds40", "bilinear8", "affine40", "lds2", "wide2")
    + _al("slide48_handover", "lds2", "affine2", "lds40", "bilinear8", "affine40", "wide2_b")
    + _al("tr48", "affine40", "lds2", "bilinear8", "affine2", "lds40", "wide2")
    + _al("bi48", "lds40", "lds2", "lds40", "lds2", "lds40", "wide2_b")
    # growth and shrinkage: owner buffer and pair data (persistent and sliding-window kernels, the bi-objective), the
    # trust-region records, (alpha, beta)
    + _growth("exact") + _al("slide520", "wide2", "slide40", "slide520", "latency8", "latency1")
    + _growth("bi") + _growth("tr") + _growth("affine")
    # initial states, then the same pairs without them on the same slot (the pinned mirror)
    + _al("exact40_init", "wide2", "exact40", "exact40_init", "exact40")
    # every level active, then a level skipped, on the same slot
    + _al("tr40", "affine2", "tr40_skip", "tr48", "tr40_skip", "tr40_skip")
    # thresholds and the batch-invariant setting
    + _al("threshold40", "exact2_invariant", "threshold40", "wide2")
    # pool B and back: the slots hold scratch sized and tagged for another level size, once larger (520 pairs of pool A
    # before 48 of pool B), once smaller (2 pairs of pool B before 40 of pool A)
    + _al("exact520", "slide520", "B_exact48", "B_wide2", "B_slide40", "B_wide2", "B_tr40", "B_bi2", "B_wide2",
          "exact40", "wide2", "B_wide2", "slide40", "B_slide40", "wide2")
)

# Two in flight: the long step followed by a short one of every user kind, and short ones followed by the long one.
PIPELINED = (
    ("pipe", ("long40", "long_wide2", "long40", "long_tr2", "long40", "slide40", "long40", "bi2", "long40", "affine2",
              "long40", "huber2", "long40", "lds2")),
    ("pipe", ("long_wide2", "long40", "long_tr2", "long40", "wide2", "long40")),
)

# evaluate calls between aligns (the watermark goes up, stays, and is passed by a smaller call on the larger level) and
# between an enqueue and its fetch
WITH_EVALUATE = (
    _al("exact40") + [("eval", 0)] + _al("wide2") + [("eval", 1)] + _al("slide40") + [("eval", 2)] + _al("wide2")
    + [("eval", 3)] + _al("tr40") + [("eval", 1), ("eval", 0)] + _al("bi2") + [("eval", 3), ("eval", 2)] + _al("wide2")
    + [("pipe", ("exact40", "eval:0", "wide2", "eval:1", "slide40", "eval:2", "wide2", "eval:3", "exact48"))]
    + _al("B_wide2") + [("eval", 1), ("eval", 2)] + _al("B_exact48", "B_wide2") + [("eval", 3)] + _al("wide2")
)


# the workspace grows while the watermark says "clean" (see EVAL_CALLS), before anything larger has been evaluated
EVALUATE_REGROWN = [("eval", 3), ("eval", 4)] + _al("wide2") + [("eval", 3), ("eval", 0), ("eval", 4)]


def random_sequence(seed, length):
    """`length` items drawn from the vocabulary: aligns (with a bias towards the users of the owner buffer and towards
    staying in a pool), pipelined stretches of two to four steps, evaluate calls.  Deterministic in (seed, length)."""
    rs = np.random.RandomState(seed)
    by_pool = {p: [n for n in DRAWN if VOCABULARY[n].pool == p] for p in POOLS}
    pool, out = "A", []

    def draw():
        names = by_pool[pool]
        weights = np.array([1.0 if VOCABULARY[n].user == "none" else 2.0 for n in names])
        weights[[len(VOCABULARY[n].which) > 100 for n in names]] *= 0.5
        return names[rs.choice(len(names), p=weights / weights.sum())]

    while len(out) < length:
        u = rs.rand()
        if u < 0.08:
            pool = "B" if pool == "A" else "A"
            out.append(("align", draw()))
        elif u < 0.20:
            out.append(("eval", int(rs.randint(len(EVAL_CALLS)))))
        elif u < 0.32:
            stretch = [draw() for _ in range(int(rs.randint(2, 5)))]
            if rs.rand() < 0.5:
                stretch.insert(int(rs.randint(1, len(stretch))), f"eval:{int(rs.randint(len(EVAL_CALLS)))}")
            out.append(("pipe", tuple(stretch)))
        else:
            out.append(("align", draw()))
    return out


RANDOM_SEEDS = (20251, 20252)
RANDOM_LENGTH = 60


def step_names(sequence):
    """The step of every enqueue of a sequence, in ticket order."""
    out = []
    for kind, what in sequence:
        if kind == "align":
            out.append(what)
        elif kind == "pipe":
            out.extend(n for n in what if not n.startswith("eval:"))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# users and transitions
# ------------------------------------------------------------------------------------------------------------------------
def classify(launches, level_pixels):
    """The user of the owner buffer that a list of launch records (AlignmentEngine.last_launches) is: from the kinds and
    from where each launch keeps its owner map (lds_bytes >= 4 n: in LDS), never from a step's label."""
    users = set()
    for r in launches:
        in_lds = r["lds_bytes"] >= 4 * max(level_pixels[l] for l in r["levels"])
        if r["kind"] == "wide":
            users.add("wide")
        elif r["kind"] in ("slide", "slide_fallback"):
            users.add("slide+fallback")
        elif r["kind"] in ("persistent", "fused") and not in_lds:
            users.add("persistent-HBM")
        elif r["kind"] == "biobjective" and not in_lds:
            users.add("bi-HBM")
        elif r["kind"] == "trust_region" and not in_lds:
            users.add("tr-HBM")
    assert len(users) <= 1, (users, launches)
    return users.pop() if users else "none"


def required_transitions():
    """(from, to, distance): every tagger -> wide, wide -> every tagger, every ordered pair of different taggers, at
    distance 1 (the other slot: hand-over, or free both and reallocate) and 2 (the same slot)."""
    return {(a, b, d) for a in USERS for b in USERS if a != b for d in (1, 2)}


def transitions(users):
    """The (from, to, distance) a list of users, one per enqueue, contains."""
    return {(users[i - d], users[i], d) for d in (1, 2) for i in range(d, len(users))}


def sits_through_non_users(users):
    """The taggers whose buffer sat through two or more non-user enqueues of its own slot (and nothing else on that slot)
    before a wide step on that slot took it."""
    found = set()
    for i, u in enumerate(users):
        if u not in TAGGERS:
            continue
        j, idle = i + 2, 0
        while j < len(users) and users[j] == "none":
            idle, j = idle + 1, j + 2
        # nobody on the OTHER slot may have needed a buffer meanwhile either, or this one could have changed hands
        if idle >= 2 and j < len(users) and users[j] == "wide" and all(x == "none" for x in users[i + 1:j]):
            found.add(u)
    return found


def growth_chains(names):
    """The step-name prefixes whose batch sizes run 40 -> 48 -> 2 -> 520 -> 40 in consecutive enqueues."""
    found = set()
    for i in range(len(names) - 4):
        five = names[i:i + 5]
        prefix = five[0][:-2]
        if five == [prefix + n for n in ("40", "48", "2", "520", "40")]:
            found.add(prefix)
    return found


# ------------------------------------------------------------------------------------------------------------------------
# anchors: the CPU checker's result for every distinct (step settings, case)
# ------------------------------------------------------------------------------------------------------------------------
def _one_ulp_of_fx(K):
    K1 = K.copy()
    K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
    return K1


@functools.lru_cache(maxsize=None)
def _pyramids(pool, problem):
    """The oracle's two-level pyramids of a problem: bit for bit the planes the device builds (test_device_pyramids_bit_exact)."""
    p = pool_problems(pool)[problem]
    cfg = oracle.make_config(num_levels=NUM_LEVELS, max_iter=[1] * NUM_LEVELS, min_grad=[0.0] * NUM_LEVELS)
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], cfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], cfg)
    return i0p, d0p, i1p, gxp, gyp


class Anchor:
    """A checker's result for one case of a step: state, its (iterations or steps per level), finite, flat (cond <= 1e5: the
    project's bar 1e-9 x max(1, cond / 1e5), capped at 1e-5, is the flat 1e-9), guard() (one ulp of fx moves the checker's
    own result by less than a quarter of the bar: (sensitivity, bar)) and check(state, report, tr, k, alpha_beta), which
    holds pair k of a device result to it by the rules of the objective's own GPU tests and returns distance / bar."""


class UnguardedExpect(Expect):
    """test_gpu_large_rotations.Expect -- the oracle's result, the conditioned bar, its check() -- without the one-ulp guard
    in the constructor: test_engine_history_cpu asserts it, once per distinct case and without a device
    (PhotometricAnchor.guard), so the GPU file does not run the oracle twice."""

    def __init__(self, ocfg, K, planes, init, **ext):
        self.max_iter = [ocfg.max_num_iterations[l] for l in range(ocfg.num_levels)]
        self.state, self.its, tr = oracle.optimize(ocfg, K, *planes, init_state=init, want_trace=True, **ext)
        self.valid = oracle.valid_pixels_per_level(tr, ocfg.num_levels)
        self.finite = bool(np.all(np.isfinite(self.state)))
        self.cond = _cond(tr)
        self.bar = min(1e-5, 1e-9 * max(1.0, self.cond / 1e5))
        self.gradient_norms = [(e["level"], float(np.linalg.norm(e["gradient"]))) for e in tr]


class PhotometricAnchor(Anchor):
    def __init__(self, step, case):
        p = pool_problems(step.pool)[case_problem(case)]
        self.kw = dict(huber_delta=huber_deltas(step), bilinear=step.bilinear, corrected=False)
        self.args = (oracle_config(step), p["K"], _pyramids(step.pool, case_problem(case)), case_init(step.pool, case, step.inits))
        self.e = UnguardedExpect(*self.args, **self.kw)
        self.finite, self.bar, self.state, self.its = self.e.finite, self.e.bar, self.e.state, self.e.its
        self.flat = self.e.cond <= 1e5

    def guard(self):
        ocfg, K, planes, init = self.args
        s1, _ = oracle.optimize(ocfg, _one_ulp_of_fx(K), *planes, init_state=init, **self.kw)
        return se3.state_distance(self.state, s1), self.bar

    def check(self, state, rep, tr, k, ab):
        self.e.check(state, rep, k)
        return se3.state_distance(state, self.state) / self.bar


class BiObjectiveAnchor(Anchor):
    def __init__(self, step, case):
        p = pool_problems(step.pool)[case_problem(case)]
        self.e = goe.BiExpect(oracle_config(step), p, case_init(step.pool, case, step.inits), guard=False)
        self.finite, self.bar, self.state, self.its = self.e.finite, self.e.bar, self.e.state, self.e.its
        self.flat = self.e.cond <= 1e5

    def guard(self):
        return self.e.sensitivity(), self.bar

    def check(self, state, rep, tr, k, ab):
        self.e.check(state, rep, k)
        return se3.state_distance(state, self.state) / self.bar


class TrustRegionAnchor(Anchor):
    def __init__(self, step, case):
        p = pool_problems(step.pool)[case_problem(case)]
        i0p, d0p, i1p, gxp, gyp = _pyramids(step.pool, case_problem(case))
        init = case_init(step.pool, case, step.inits)
        self.args = args = (oracle_config(step), p["K"], (i0p, d0p), (i1p, gxp, gyp), trust_region_options(), init)
        self.state, self.recs = tref.optimize(*args)
        self.finite = bool(np.all(np.isfinite(self.state)))
        self.flat = max(r["cond"] for r in self.recs.values()) <= 1e5
        self.margin = min((m for r in self.recs.values() for m in r["margins"]), default=1.0)
        self.its = [self.recs[L]["steps"] if L in self.recs else 0 for L in range(NUM_LEVELS)]
        self.bar = gtr.POSE_TOL

    def guard(self):
        s1, _ = tref.optimize(self.args[0], _one_ulp_of_fx(self.args[1]), *self.args[2:])
        return float(np.abs(self.state - s1).max()), self.bar

    def check(self, state, rep, tr, k, ab):
        assert self.margin > gtr.MARGIN, "a decision of the checker is knife-edge: choose other inputs"
        return gtr.compare_pair(k, state, rep, tr, self.state, self.recs, NUM_LEVELS)


class AffineAnchor(Anchor):
    def __init__(self, step, case):
        p = pool_problems(step.pool)[case_problem(case)]
        pyr = list(zip(*_pyramids(step.pool, case_problem(case))))
        cfg = dict(num_levels=NUM_LEVELS, lam=[1.0] * NUM_LEVELS, max_iter=list(step.max_iter), min_grad=list(step.min_grad))
        init = case_init(step.pool, case, step.inits)
        self.args = (pyr, p["K"], cfg, init)
        self.ref = ar.optimize(*self.args)
        self.state, self.its = self.ref["state"], self.ref["iterations"]
        self.finite = bool(np.all(np.isfinite(self.state)))
        self.bar = ar.pose_bar(self.ref["cond"], self.state)
        self.flat = self.ref["cond"] <= 1e5

    def guard(self):
        pyr, K, cfg, init = self.args
        return float(np.abs(self.state - ar.optimize(pyr, _one_ulp_of_fx(K), cfg, init)["state"]).max()), self.bar

    def check(self, state, rep, tr, k, ab):
        import test_gpu_affine
        test_gpu_affine._compare(state, ab, rep, self.ref, NUM_LEVELS)
        return float(np.abs(np.concatenate([state, ab]) - self.state).max()) / self.bar


ANCHORS = {"photometric": PhotometricAnchor, "biobjective": BiObjectiveAnchor, "trust_region": TrustRegionAnchor,
           "affine": AffineAnchor}


def anchor_key(step, case):
    """What the checker's result depends on: not the batch, the policies or the forms."""
    return (step.pool, step.objective, step.bilinear, step.huber, step.max_iter, step.min_grad, step.inits and case < 3, case)


_anchors = {}


def anchor(step, case):
    """The (cached) checker result of one case of a step; steps that differ in batch or form only share it."""
    key = anchor_key(step, case)
    if key not in _anchors:
        _anchors[key] = ANCHORS[step.objective](step, case)
    return _anchors[key]


def anchor_keys():
    """{key: (step, case)} over the whole vocabulary: every distinct checker run."""
    out = {}
    for step in VOCABULARY.values():
        for case in sorted(set(step.which)):
            out.setdefault(anchor_key(step, case), (step, case))
    return out
