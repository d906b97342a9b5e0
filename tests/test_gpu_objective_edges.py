"""The bi-objective (gn_biobjective_kernel.hip) and trust-region (gn_trust_region_kernel.hip) kernels at their edges,
against their CPU checkers (tests/biobjective_ref.py, tests/trust_region_ref.py); run with -m gpu on an MI355X.

* initial states in every branch of write_pose_constants (tests/edge_states.py) and true in-plane motions up to 0.9 rad,
  in each of the three geometries of both kernels: 256 threads with the owner map in LDS, 512 threads with it in LDS, and
  512 threads with it in HBM;
* a NaN / inf initial angle in one pair of a launch;
* more than 1023 evaluations in one level, so that the owner-map tags (kept in LDS as well as in HBM) wrap and the map is
  wiped;
* the trust region's remaining terminations (MIN_RADIUS, INVALID_STEP, EVALUATION_FAILED) and rejected steps;
* strips one to five pixels wide, and a level of fewer than 64 pixels (one partial chunk).
Every case asserts that it reached its edge: the launch kind and thread count, the wrap, or the termination.
"""
import numpy as np
import pytest

import biobjective_ref as bref
import edge_states
import test_gpu_trust_region as gtr
import trust_region_ref as tref
from test_gpu_large_rotations import _cond

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

# (size, threads, owner map in LDS) of the three geometries of both kernels
GEOMETRIES = [((80, 60), 256, True), ((200, 150), 512, True), ((320, 240), 512, False)]
GEOMETRY_IDS = ["lds256_80x60", "lds512_200x150", "hbm_320x240"]
GOOD = np.array([0.01, -0.02, 0.015, 0.02, -0.01, 0.015])
BAD = ((0, np.nan), (1, np.inf), (2, -np.inf))          # (angle, value): NaN yaw, +inf pitch, -inf roll
BAD_AT = 4


def _assert_geometry(launches, kind, threads, in_lds, n):
    """One launch of `kind` with `threads` threads, its owner map (4 bytes per pixel) in LDS or not."""
    assert [(r["kind"], r["threads"]) for r in launches] == [(kind, threads)], launches
    assert (launches[0]["lds_bytes"] >= 4 * n) == in_lds, (launches[0]["lds_bytes"], n)


def _strip(w, h, seed=33):
    """A w x h pair: rendered at that size, or a narrow strip of a 64-pixel-wide render (as test_level_geometries), with
    the principal point moved with the crop so that the strip's pixels warp where the render's do."""
    if w >= 8:
        return synthetic.make_pair(seed, w, h, holes=0.02)
    p = synthetic.make_pair(seed, 64, h, holes=0.02)
    for k in ("gray0", "depth0", "gray1", "depth1"):
        p[k] = np.ascontiguousarray(p[k][:, 30:30 + w])
    p["K"] = p["K"].copy()
    p["K"][0, 2] -= 30.0
    return p


# ------------------------------------------------------------------------------------------------------------------------
# bi-objective
# ------------------------------------------------------------------------------------------------------------------------
def _bi_cfgs(max_iter, min_grad=None):
    nl = len(max_iter)
    mg = [0.0] * nl if min_grad is None else min_grad
    return (native.make_config(num_levels=nl, max_iter=max_iter, min_grad=mg),
            oracle.make_config(num_levels=nl, max_iter=max_iter, min_grad=mg))


def _bi_engine(ncfg, ps):
    h, w = ps[0]["gray0"].shape
    e = odometry.AlignmentEngine(0)
    e.set_config(ncfg)
    e.set_intrinsic_matrix(ps[0]["K"])
    e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
    e.reserve_frames(2 * len(ps), w, h)
    for k, p in enumerate(ps):
        e.upload_frame(2 * k, p["gray0"], p["depth0"], native.ROLE_SOURCE)
        e.upload_frame(2 * k + 1, p["gray1"], p["depth1"], native.ROLE_TARGET)
    return e


class BiExpect:
    """The bi-objective checker's result for one case, the conditioned pose bar of test_gpu_large_rotations.Expect
    (1e-9 x max(1, cond(H) / 1e5)) and the same well-posedness guard: one ulp of fx moves the checker's own result by
    less than a quarter of the bar."""

    def __init__(self, ocfg, p, init, min_depth=0.3, max_depth=5.0, plane_max_depth=5.0, guard=True):
        """min_depth / max_depth: the depth gate in force at the alignment; plane_max_depth: the max depth in force when
        the target was uploaded (its depth-gradient planes).  guard=False leaves the well-posedness
        check to the caller (sensitivity())."""
        self.max_iter = [ocfg.max_num_iterations[l] for l in range(ocfg.num_levels)]
        self._args = (ocfg, p["K"], oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg),
                      bref.target_planes(p["gray1"], p["depth1"], ocfg, plane_max_depth), init, min_depth, max_depth)
        self.state, self.its, self.valid, self.flags, tr = bref.optimize(*self._args)
        self.finite = bool(np.all(np.isfinite(self.state)))
        self.cond = _cond([dict(hessian=t["H"]) for t in tr])
        self.bar = min(1e-5, 1e-9 * max(1.0, self.cond / 1e5))
        if self.finite and guard:
            sens = self.sensitivity()
            assert sens < 0.25 * self.bar, f"chaotic case: one ulp of fx moves the checker by {sens:.3e}, bar {self.bar:.1e}"

    def sensitivity(self):
        """How far the checker's own pose moves when fx changes by one ulp."""
        ocfg, K, src, tgt, init, lo, hi = self._args
        K1 = K.copy()
        K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
        s1 = bref.optimize(ocfg, K1, src, tgt, init, lo, hi)[0]
        return se3.state_distance(self.state, s1) if np.all(np.isfinite(s1)) else np.inf

    def check(self, state, rep, what):
        nl = len(self.its)
        its = list(rep.iterations[:nl])
        assert list(rep.valid_pixels[:nl]) == self.valid, (what, list(rep.valid_pixels[:nl]), self.valid)
        if not self.finite:
            # the device stops at the first non-finite state; the checker does too, so the counts are at most its
            assert rep.flags & native.PAIR_NONFINITE and not np.all(np.isfinite(state)), (what, rep.flags, state)
            assert all(d <= o for d, o in zip(its, self.its)), (what, its, self.its)
            return
        assert its == self.its, (what, its, self.its)
        assert rep.flags == self.flags, (what, rep.flags, self.flags)
        d = se3.state_distance(state, self.state)
        assert d < self.bar, (what, d, self.bar)


@pytest.mark.parametrize("size,threads,in_lds", GEOMETRIES, ids=GEOMETRY_IDS)
def test_biobjective_initial_states_in_every_branch(size, threads, in_lds):
    """The 32 initial states of edge_states, three fixed iterations, nine pairs per launch, in each geometry."""
    w, h = size
    p = synthetic.make_pair(61, w, h, holes=0.02, trans=0.01, rot=0.004)
    ncfg, ocfg = _bi_cfgs([3])
    inits = edge_states.initial_states()
    expect = [BiExpect(ocfg, p, s) for s in inits]
    assert any(not e.finite or e.valid[0] < w * h // 4 for e in expect)          # some states see (almost) nothing
    assert sum(e.finite for e in expect) >= 24
    with _bi_engine(ncfg, [p]) as e:
        for g in range(0, len(inits), 9):
            idx = [(g + k) % len(inits) for k in range(9)]
            s, reps = e.align_pairs([0] * 9, [1] * 9, init_states=np.stack([inits[i] for i in idx]), want_reports=True)
            _assert_geometry(e.last_launches(), "biobjective", threads, in_lds, w * h)
            for k, i in enumerate(idx):
                expect[i].check(s[k], reps[k], (size, i, inits[i][3:]))


def test_biobjective_large_in_plane_motions():
    """Rendered pairs under in-plane rotations of 0.7 and 0.9 rad, started near the truth, ten iterations."""
    w, h = 160, 120
    ncfg, ocfg = _bi_cfgs([10])
    for j, m in enumerate(edge_states.MOTIONS[1:]):
        p = synthetic.render_pair_with_motion(70 + j, w, h, m)
        init = p["motion"] + edge_states.NEAR
        ex = BiExpect(ocfg, p, init)
        assert ex.finite and abs(ex.state[3] - m[3]) < 0.05, (ex.state, m)
        with _bi_engine(ncfg, [p]) as e:
            s, reps = e.align_pairs([0] * 9, [1] * 9, init_states=np.tile(init, (9, 1)), want_reports=True)
            assert [r["kind"] for r in e.last_launches()] == ["biobjective"]
        for k in range(9):
            ex.check(s[k], reps[k], (m[3], k))
            assert np.array_equal(s[k], s[0])


@pytest.mark.parametrize("size,threads,in_lds,pairs", [((80, 60), 256, True, 9), ((320, 240), 512, False, 40)],
                         ids=["lds256_80x60", "hbm_320x240"])
def test_biobjective_non_finite_initial_angle_in_one_pair(size, threads, in_lds, pairs):
    """NaN yaw, +inf pitch, -inf roll as the initial state of pair 4: it ends non-finite, flagged NONFINITE, with no
    contributing pixel; every other pair is bit for bit what it is without it, and matches the checker."""
    w, h = size
    p = synthetic.make_pair(64, w, h, holes=0.02, trans=0.01, rot=0.004)
    ncfg, ocfg = _bi_cfgs([3])
    inits = np.tile(GOOD, (pairs, 1))
    results = []
    with _bi_engine(ncfg, [p]) as e:
        clean = e.align_pairs([0] * pairs, [1] * pairs, init_states=inits)
        for axis, bad in BAD:
            st = inits.copy()
            st[BAD_AT, 3 + axis] = bad
            s, reps = e.align_pairs([0] * pairs, [1] * pairs, init_states=st, want_reports=True)
            _assert_geometry(e.last_launches(), "biobjective", threads, in_lds, w * h)
            results.append((st[BAD_AT], s, reps))
    e_good = BiExpect(ocfg, p, GOOD)
    for st, s, reps in results:
        e_bad = BiExpect(ocfg, p, st)
        assert not e_bad.finite and e_bad.valid == [0]
        e_bad.check(s[BAD_AT], reps[BAD_AT], ("bad", st[3:]))
        assert reps[BAD_AT].valid_pixels[0] == 0
        for k in range(pairs):
            if k != BAD_AT:
                assert np.array_equal(s[k], clean[k]), (k, st[3:])
                assert reps[k].flags & native.PAIR_NONFINITE == 0
                e_good.check(s[k], reps[k], ("good", k, st[3:]))


@pytest.mark.parametrize("size,threads,in_lds,seed", [GEOMETRIES[0] + (68,), GEOMETRIES[2] + (65,)],
                         ids=["lds256_80x60", "hbm_320x240"])
def test_biobjective_owner_tags_wrap(size, threads, in_lds, seed):
    """1040 fixed iterations of 40 pairs: the owner-map tags run through their period of 1023 and the map is wiped once;
    the pose stays within 1e-9 of the checker and every copy is the same bits.  (The bi-objective step does not settle:
    the pose still moves after 1000 iterations.  The seeds are ones on which one ulp of fx moves the checker's pose by
    less than a quarter of the bar after 1040 iterations, as the guard below asserts; on others, such as seed 65 at
    80x60, it moves by 7e-8.)"""
    w, h = size
    p = synthetic.make_pair(seed, w, h, holes=0.02)
    ncfg, ocfg = _bi_cfgs([1040])
    with _bi_engine(ncfg, [p]) as e:
        s, reps = e.align_pairs([0] * 40, [1] * 40, want_reports=True)
        _assert_geometry(e.last_launches(), "biobjective", threads, in_lds, w * h)
    src = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    tgt = bref.target_planes(p["gray1"], p["depth1"], ocfg, 5.0)
    es, its, valid, flags, _ = bref.optimize(ocfg, p["K"], src, tgt)
    K1 = p["K"].copy()
    K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
    assert se3.state_distance(es, bref.optimize(ocfg, K1, src, tgt)[0]) < 0.25e-9      # well-posed for the 1e-9 bar
    assert its == [1040]
    for k in range(40):
        assert list(reps[k].iterations[:1]) == [1040] and list(reps[k].valid_pixels[:1]) == valid, k
        assert reps[k].flags == flags == 0
        assert np.array_equal(s[k], s[0]), k
    assert se3.state_distance(s[0], es) < 1e-9, se3.state_distance(s[0], es)


@pytest.mark.parametrize("w,h", [(1, 40), (2, 33), (3, 17), (4, 64), (5, 70), (75, 53)])
def test_biobjective_tiny_and_odd_levels(w, h):
    """Strips one to five pixels wide and a 75x53 level: the target's depth planes, depth gradients (Scharr) and gain
    against the checker's, and alignments from three states against it."""
    p = _strip(w, h)
    ncfg, ocfg = _bi_cfgs([3])
    rs = np.random.RandomState(w * 1000 + h)
    states = [np.zeros(6), p["motion"], rs.uniform(-0.02, 0.02, 6)]
    with _bi_engine(ncfg, [p]) as e:
        tp = bref.target_planes(p["gray1"], p["depth1"], ocfg, 5.0)
        _, d, _, _ = e.get_level_planes(1, 0)
        assert np.array_equal(d, tp["d1"][0])
        gx, gy = e.get_level_depth_gradients(1, 0)
        assert np.array_equal(gx, tp["dgx"][0]) and np.array_equal(gy, tp["dgy"][0])
        assert abs(e.get_level_depth_gain(1, 0) - tp["gain"][0]) <= 1e-14 * abs(tp["gain"][0])
        s, reps = e.align_pairs([0] * 3, [1] * 3, init_states=np.stack(states), want_reports=True)
        assert [r["kind"] for r in e.last_launches()] == ["biobjective"]
    for k, st in enumerate(states):
        BiExpect(ocfg, p, st).check(s[k], reps[k], (w, h, k))


# ------------------------------------------------------------------------------------------------------------------------
# trust region
# ------------------------------------------------------------------------------------------------------------------------
def _tr_setup(max_iter, **opts):
    """The only-level-0 Ceres fixture with max_num_iterations and per-level options of level 0 replaced."""
    cfg, opt = gtr._fixture("config_only_level_0_ceres.yml")
    cfg.max_num_iterations[0] = max_iter
    for f, v in opts.items():
        getattr(opt, f)[0] = v
    return cfg, opt


def _tr_levels(ps, cfg, opt, inits=None):
    """The checker's (state, records) of every pair."""
    ocfg = tref.oracle_config(cfg)
    return [tref.align(ocfg, p["K"], p["gray0"], p["depth0"], p["gray1"], opt, None if inits is None else inits[k])
            for k, p in enumerate(ps)]


@pytest.mark.parametrize("size,threads,in_lds", GEOMETRIES, ids=GEOMETRY_IDS)
def test_trust_region_initial_states_in_every_branch(size, threads, in_lds):
    """The 32 initial states of edge_states and three true in-plane motions of 0.5 to 0.9 rad, five LM steps each, through
    test_gpu_trust_region._check (steps, accepted steps, terminations, costs, radii, flags; decisions not knife-edge),
    in each geometry.  The pose bar is 1e-9 x max(1, |x|): from pitch 0.80 at 200x150 the solve runs off to 95 m, where
    the two sides agree to 2.4e-9."""
    w, h = size
    p = synthetic.make_pair(61, w, h, holes=0.02, trans=0.01, rot=0.004)
    moving = [synthetic.render_pair_with_motion(70 + j, w, h, m) for j, m in enumerate(edge_states.MOTIONS)]
    inits = edge_states.initial_states() + [q["motion"] + edge_states.NEAR for q in moving]
    ps = [p] * 32 + moving
    cfg, opt = _tr_setup(5)
    tr = gtr._check(cfg, opt, ps, np.stack(inits), relative_pose=True)
    _assert_geometry(gtr.LAUNCHES, "trust_region", threads, in_lds, w * h)
    assert np.any(tr["rows"][:, 0] < w * h // 4)                         # some states see (almost) nothing
    assert np.sum(tr["accepted"][:, 0] > 0) >= 20


@pytest.mark.parametrize("size,threads,in_lds,pairs", [(g[0], g[1], g[2], 40 if not g[2] else 9) for g in GEOMETRIES],
                         ids=GEOMETRY_IDS)
def test_trust_region_non_finite_initial_angle_in_one_pair(size, threads, in_lds, pairs):
    """NaN yaw, +inf pitch, -inf roll as the initial state of pair 4: no pixel warps, the first system is finite and zero,
    and the level ends without a step with the state as given -- flagged NONFINITE (the state is not finite), with 0
    rows and the checker's termination; every other pair is bit for bit what it is without it, and matches the checker."""
    w, h = size
    p = synthetic.make_pair(64, w, h, holes=0.02, trans=0.01, rot=0.004)
    cfg, opt = _tr_setup(5)
    inits = np.tile(GOOD, (pairs, 1))
    results = []
    with gtr._engine(cfg, opt, p["K"]) as e:
        gtr._upload(e, [p])
        clean = e.align_pairs([0] * pairs, [1] * pairs, init_states=inits)
        tr_clean = e.trust_region_reports(pairs)
        for axis, bad in BAD:
            st = inits.copy()
            st[BAD_AT, 3 + axis] = bad
            s, reps = e.align_pairs([0] * pairs, [1] * pairs, init_states=st, want_reports=True)
            _assert_geometry(e.last_launches(), "trust_region", threads, in_lds, w * h)
            results.append((st[BAD_AT], s, reps, e.trust_region_reports(pairs)))
    (xg, rg), = _tr_levels([p], cfg, opt, [GOOD])
    assert min(rg[0]["margins"]) > gtr.MARGIN and rg[0]["noise_from"] is None
    for st, s, reps, tr in results:
        (xb, rb), = _tr_levels([p], cfg, opt, [st])
        assert rb[0]["rows"] == 0 and rb[0]["termination"] == native.TR_GRADIENT and tref.pair_flags(xb, rb) == 5
        assert np.array_equal(s[BAD_AT], st, equal_nan=True), (s[BAD_AT], st)
        assert reps[BAD_AT].flags == tref.pair_flags(xb, rb), (st[3:], reps[BAD_AT].flags)
        assert reps[BAD_AT].valid_pixels[0] == 0 and reps[BAD_AT].iterations[0] == rb[0]["steps"] == 0
        assert tr["termination"][BAD_AT, 0] == rb[0]["termination"] and tr["rows"][BAD_AT, 0] == 0
        for k in range(pairs):
            if k == BAD_AT:
                continue
            assert np.array_equal(s[k], clean[k]) and tr[k:k + 1].tobytes() == tr_clean[k:k + 1].tobytes(), (k, st[3:])
            assert reps[k].flags == tref.pair_flags(xg, rg) == 0, (k, reps[k].flags)
            assert np.abs(s[k] - xg).max() <= gtr.POSE_TOL
            assert tr["steps"][k, 0] == rg[0]["steps"] and tr["accepted"][k, 0] == rg[0]["accepted"]
            assert tr["termination"][k, 0] == rg[0]["termination"] and tr["rows"][k, 0] == rg[0]["rows"]


@pytest.mark.parametrize("size,threads,in_lds", [GEOMETRIES[0], GEOMETRIES[2]], ids=["lds256_80x60", "hbm_320x240"])
def test_trust_region_owner_tags_wrap(size, threads, in_lds):
    """1040 LM steps, 1041 evaluations of 40 pairs: the owner-map tags run through their period of 1023 and the map is
    wiped once.  The function and gradient tolerances and the minimum radius are below zero and the parameter tolerance
    is 0; the radius is capped at 0.01 so that every step moves the state by far more than its rounding (the parameter
    test, which a step that rounds away would meet even at tolerance 0, never passes, and every decision is
    conditioned): only the iteration limit stops the level.  At the device's state the checker's rows and cost are the
    device's, and the pose is the checker's within 1e-9."""
    w, h = size
    p = synthetic.make_pair(91, w, h, holes=0.02)
    cfg, opt = _tr_setup(1040, function_tolerance=-1.0, gradient_tolerance=-1.0, min_trust_region_radius=-1.0,
                         parameter_tolerance=0.0, initial_trust_region_radius=0.01, max_trust_region_radius=0.01)
    with gtr._engine(cfg, opt, p["K"]) as e:
        gtr._upload(e, [p])
        s, reps = e.align_pairs([0] * 40, [1] * 40, want_reports=True)
        tr = e.trust_region_reports(40)
        _assert_geometry(e.last_launches(), "trust_region", threads, in_lds, w * h)
    assert tr["termination"][0, 0] == native.TR_MAX_ITERATIONS and tr["steps"][0, 0] == 1040    # 1041 evaluations
    for k in range(40):
        assert np.array_equal(s[k], s[0]) and tr[k:k + 1].tobytes() == tr[0:1].tobytes(), k
    ocfg = tref.oracle_config(cfg)
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    ev = tref.evaluate(i0p[0], d0p[0], i1p[0], gxp[0], gyp[0], 0, p["K"], s[0])
    assert ev["rows"] == reps[0].valid_pixels[0] == tr["rows"][0, 0]
    assert abs(ev["cost"] - tr["final_cost"][0, 0]) <= 1e-12 * ev["cost"], (ev["cost"], tr["final_cost"][0, 0])
    (xs, recs), = _tr_levels([p], cfg, opt)
    rec = recs[0]
    assert rec["steps"] == 1040 and rec["noise_from"] is None and min(rec["margins"]) > gtr.MARGIN
    assert tr["accepted"][0, 0] == rec["accepted"]
    assert np.abs(s[0] - xs).max() <= 1e-9, (s[0], xs)


def _tr_compare_terminal(e, p, cfg, opt, init, planes=None):
    """Align one pair on the device and compare its record with the checker's, decision for decision, without the
    margin guard (for levels whose only decision is exact: a zero model cost change, a non-finite first evaluation)."""
    s, reps = e.align_pairs([0], [1], init_states=init[None], want_reports=True)
    tr = e.trust_region_reports(1)
    assert [r["kind"] for r in e.last_launches()] == ["trust_region"]
    if planes is None:
        (xs, recs), = _tr_levels([p], cfg, opt, [init])
    else:
        i0, d0, i1, gx, gy = planes
        xs, rec = tref.optimize_level(lambda x: tref.evaluate(i0, d0, i1, gx, gy, 0, p["K"], x), init,
                                      cfg.max_num_iterations[0], **tref.level_options(opt, 0))
        recs = {0: rec}
    rec = recs[0]
    for f in ("steps", "accepted", "termination", "rows"):
        assert tr[f][0, 0] == rec[f], (f, tr[f][0, 0], rec[f])
    assert np.array_equal(s[0], xs)
    assert reps[0].flags == tref.pair_flags(xs, recs), reps[0].flags
    return s[0], reps[0], tr, rec


def test_trust_region_min_radius():
    """A minimum radius above the initial one: the level stops at its first loop head, after the gradient test."""
    p = synthetic.make_pair(7, 200, 150)
    cfg, opt = _tr_setup(10, min_trust_region_radius=1e5)
    tr = gtr._check(cfg, opt, [p])
    assert tr["termination"][0, 0] == native.TR_MIN_RADIUS and tr["steps"][0, 0] == 0


def test_trust_region_invalid_step():
    """Every source depth invalid: no row, a zero system, a zero step and a zero model cost change (the gradient test is
    switched off, else it would stop the level first)."""
    p = synthetic.make_pair(7, 200, 150)
    p["depth0"] = np.zeros_like(p["depth0"])
    cfg, opt = _tr_setup(10, gradient_tolerance=-1.0)
    with gtr._engine(cfg, opt, p["K"]) as e:
        gtr._upload(e, [p])
        s, rep, tr, rec = _tr_compare_terminal(e, p, cfg, opt, GOOD)
    assert rec["termination"] == native.TR_INVALID_STEP and rec["steps"] == 1 and rec["rows"] == 0
    assert rep.flags == native.PAIR_RANK_DEFICIENT and tr["final_cost"][0, 0] == 0.0
    assert np.array_equal(s, GOOD)


def test_trust_region_evaluation_failed():
    """A NaN block in the target intensity: the first evaluation is not finite.  Flags NONFINITE, gradient norm NaN, the
    state left at its initial value."""
    p = synthetic.make_pair(36, 160, 120)
    cfg, opt = _tr_setup(10)
    with gtr._engine(cfg, opt, p["K"]) as e:
        gtr._upload(e, [p])
        i1, _, gx, gy = e.get_level_planes(1, 0)
        i1[50:60, 70:90] = np.nan
        e.set_level_planes(1, 0, intensity=i1)
        i0, d0, _, _ = e.get_level_planes(0, 0)
        s, rep, tr, rec = _tr_compare_terminal(e, p, cfg, opt, GOOD, planes=(i0, d0, i1, gx, gy))
    assert rec["termination"] == native.TR_EVALUATION_FAILED and rec["steps"] == 0
    assert rep.flags & native.PAIR_NONFINITE and np.isnan(rep.gradient_norm)
    assert np.array_equal(s, GOOD)


def test_trust_region_rejected_steps():
    """From zero with the fixture's radius, ten steps of which the checker rejects some: equal counts on both sides."""
    p = synthetic.make_pair(7, 200, 150)
    cfg, opt = _tr_setup(10)
    tr = gtr._check(cfg, opt, [p])
    assert tr["termination"][0, 0] == native.TR_MAX_ITERATIONS                       # no terminal step
    assert tr["steps"][0, 0] - tr["accepted"][0, 0] >= 1, (tr["steps"][0, 0], tr["accepted"][0, 0])


@pytest.mark.parametrize("w,h", [(1, 40), (2, 33), (3, 17), (4, 64), (5, 70), (75, 53)])
def test_trust_region_tiny_and_odd_levels(w, h):
    """Strips one to five pixels wide (linear_axis at W of 1 and 2: both taps clamped, or one interior pair) and a 75x53
    level, three initial states each, through _check."""
    p = _strip(w, h)
    rs = np.random.RandomState(w * 1000 + h)
    inits = np.stack([np.zeros(6), p["motion"], rs.uniform(-0.02, 0.02, 6)])
    cfg, opt = _tr_setup(5)
    tr = gtr._check(cfg, opt, [p] * 3, inits)
    assert gtr.LAUNCHES[0]["threads"] == 256
    if (w, h) == (3, 17):
        assert np.all(tr["rows"][:2, 0] > 0)                          # 51 pixels: one partial chunk, with rows in it

