"""The inverse-compositional kernel (gn_inverse_kernel.hip) where tests/test_gpu_inverse.py does not reach:
the second trip of its persistent loop with (R, t), the flags and the prefetched source values living across it; rows and
clamped taps at exact positions and depth exactly at the gate; the three regimes of its Exp and atan2 up to 3 rad, from one
iteration whose step length sets |omega|; initial states in every branch of the device's sin / cos; step lengths other
than 1 that differ between the levels; fy != fx with a principal point off the half-integer grid; systems of exactly 5, 6
and 7 rows, summed inside one wave and across all four; a skipped level between two that run and a level of 50 iterations.
The reference of every comparison is tests/inverse_ref.py in fp64 on the planes as the device holds them; the bars are
test_gpu_inverse._compare's (iterations, valid_pixels and flags exact, the pose to inverse_ref.pose_bar, the gradient norm
to 1e-9 relative).  Every fixture (tests/inverse_edges.py) is chosen to hold the flat bar, to stay clear of its gradient
thresholds and to end clear of atan2's branch cut; tests/test_inverse_edges_cpu.py asserts that without a device."""
import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

import edge_states
import inverse_edges as ie
import inverse_ref as ir
# (helpers of the first inverse GPU file, used as they are so that both files hold the device to the same bars)
from test_gpu_inverse import INVERSE, MARGIN_FLOOR, _bits, _compare, _device_pyramid

assert ie.MARGIN_FLOOR == MARGIN_FLOOR

pytestmark = pytest.mark.gpu

BOTH = ir.PAIR_RANK_DEFICIENT | ir.PAIR_NONFINITE


def _engine(K, w, h, frames, mi, mg=None, depth_range=None, lam=None):
    nl = len(mi)
    eng = odometry.AlignmentEngine()
    eng.set_config(native.make_config(num_levels=nl, max_iter=mi, min_grad=mg if mg else [0.0] * nl, lam=lam))
    eng.set_objective(INVERSE)
    eng.set_intrinsic_matrix(K)
    if depth_range is not None:
        eng.set_depth_range(*depth_range)
    eng.reserve_frames(frames, w, h)
    return eng


def _upload(eng, pairs):
    """Pair i: source frame 2 i, target frame 2 i + 1."""
    for i, p in enumerate(pairs):
        eng.upload_frame(2 * i, p["gray0"], p["depth0"])
        eng.upload_frame(2 * i + 1, p["gray1"], p["depth1"])


def _set_planes(eng, i, planes):
    """Pair i of one level, plane by plane: the source's four planes, the target's intensity."""
    i0, d0, gx0, gy0, i1 = planes
    eng.set_level_planes(2 * i, 0, intensity=i0, depth=d0, grad_x=gx0, grad_y=gy0)
    eng.set_level_planes(2 * i + 1, 0, intensity=i1)


def _align(eng, which, inits=None):
    """Pairs which[k] of _upload in one enqueue -> (states, reports); every launch is the inverse kernel's."""
    which = np.asarray(which, dtype=int)
    s, reps = eng.align_pairs(2 * which, 2 * which + 1, init_states=inits, want_reports=True)
    assert {l["kind"] for l in eng.last_launches()} == {"inverse"}
    return s, reps


def _record(s, rep, nl):
    """Everything a pair reports, for bit-for-bit comparison."""
    return (_bits(s), list(rep.iterations[:nl]), list(rep.valid_pixels[:nl]), int(rep.flags), _bits([rep.gradient_norm]))


def _hold(part, what, s, rep, ref, nl):
    """test_gpu_inverse._compare under the flat bar, the keep-out margins on the planes the device holds, and the
    distance / bar of the pair printed for DESIGN.md §20's table."""
    _compare(s, rep, ref, nl, expect_flat=True)
    if np.all(np.isfinite(ref["state"])):
        assert ie.clear_of_the_cuts(ref["state"]), ref["state"]
        ratio = np.abs(s - ref["state"]).max() / ir.pose_bar(ref["cond"], ref["state"])
        print(f"part {part} {what}: distance / bar {ratio:.3g}, cond {ref['cond']:.2e}")
        return ratio
    return 0.0


# ---- A. more pairs than resident workgroups ----------------------------------------------------------------------------
def test_inverse_work_queue():
    """N = 3 G + 5 pairs (G: the persistent grid of a large enqueue) drawn from four tiny pairs that end after different
    numbers of iterations, one of them with an all-NaN source depth: every workgroup takes several trips through the
    kernel's pair loop.  Every position equals, bit for bit, the same pair aligned alone -- a flag, an (R, t), a row count
    or a prefetched source value that survived from one pair to the next on a workgroup would break that somewhere -- on
    three enqueues in a row, and a second list starts every pair from its own non-zero state."""
    nl = ie.WQ_LEVELS
    pairs = ie.work_queue_pairs()
    K = pairs[0]["K"]
    cfg = ie.cfg(ie.WQ_MAX_ITER, ie.WQ_MIN_GRAD)
    worst = 0.0
    with _engine(K, ie.WQ_W, ie.WQ_H, 8, ie.WQ_MAX_ITER, ie.WQ_MIN_GRAD) as eng:
        _upload(eng, pairs)
        pyr = [_device_pyramid(eng, 2 * i, 2 * i + 1, nl, ie.WQ_MAX_ITER) for i in range(4)]
        alone = []
        for i in range(4):                                      # the 1-pair probes: held to the checker
            s, reps = _align(eng, [i])
            assert all(l["workgroups"] == 1 for l in eng.last_launches())
            ref = ir.optimize(pyr[i], K, cfg)
            worst = max(worst, _hold("A", f"pair {i}", s[0], reps[0], ref, nl))
            alone.append(_record(s[0], reps[0], nl))
            assert np.all(np.isnan(s[0])) == (i == ie.WQ_D)
        assert alone[ie.WQ_D][1:4] == ([1, 1], [0, 0], BOTH)
        assert len({repr(a) for a in alone}) == 4
        assert len({repr(a[1]) for a in alone[:ie.WQ_D]}) >= 2      # by threshold, at counts that are not all equal
        assert all(1 < it < m for a in alone[:ie.WQ_D] for it, m in zip(a[1], ie.WQ_MAX_ITER))
        _align(eng, [0] * 4096)
        G = eng.last_launches()[0]["workgroups"]
        N = 3 * G + 5
        which = ie.work_queue_list(N)
        assert set(which.tolist()) == {0, 1, 2, 3}
        for run in range(3):
            s, reps = _align(eng, which)
            launches = eng.last_launches()
            print(f"run {run}: N = {N}, grid {launches[0]['workgroups']} (G = {G})")
            assert len(launches) == nl and all(l["workgroups"] == G < N for l in launches)
            for k in range(N):
                assert _record(s[k], reps[k], nl) == alone[which[k]], (run, k, which[k])

        # every pair from its own non-zero state: states[pair] is read per pair inside the loop
        N2 = 520
        states, pick = ie.work_queue_inits(N2)
        which2 = ie.work_queue_list(N2, seed=2)
        combos = sorted({(int(a), int(b)) for a, b in zip(which2, pick)})
        assert len({b for _, b in combos}) == ie.WQ_INITS == 6
        alone2 = {}
        for a, b in combos:
            s, reps = _align(eng, [a], states[b][None])
            ref = ir.optimize(pyr[a], K, cfg, init_pose=states[b])
            worst = max(worst, _hold("A", f"pair {a} from state {b}", s[0], reps[0], ref, nl))
            alone2[(a, b)] = _record(s[0], reps[0], nl)
        s, reps = _align(eng, which2, states[pick])
        assert all(l["workgroups"] < N2 for l in eng.last_launches())      # a second trip somewhere
        for k in range(N2):
            assert _record(s[k], reps[k], nl) == alone2[(int(which2[k]), int(pick[k]))], (k, which2[k], pick[k])
        assert len({repr(v) for (a, b), v in alone2.items() if a != ie.WQ_D}) == len([c for c in combos if c[0] != ie.WQ_D])
    print(f"part A: largest distance / bar {worst:.3g}")


# ---- B. exact positions ------------------------------------------------------------------------------------------------
EXACT_CASES = [(w, h, s, r) for (w, h), shifts in ie.EXACT_SIZES.items() for s in shifts for r in ie.RANGES]


@pytest.mark.parametrize("w,h,shift,depth_range", EXACT_CASES,
                         ids=[f"{w}x{h}_{s:+.2f}_{r[0]}_{r[1]}" for w, h, s, r in EXACT_CASES])
def test_inverse_exact_rows_and_taps(w, h, shift, depth_range):
    """Every projected coordinate is exactly c + shift, r + shift: at +-0.5 the outermost column and row sit on -0.5 /
    W - 0.5 and are out (both comparisons are strict), at +-0.25 they are rows whose taps are clamped, at +-0.75 they are
    out; a column at min_depth and a row at max_depth are out (for the range 0.5 / 2.0 also depths 0.4 and 3.0)."""
    K, planes, state = ie.exact_problem(w, h, shift, depth_range)
    expected = ie.exact_rows(planes[1], shift)
    with _engine(K, w, h, 2, [1], depth_range=depth_range) as eng:
        _set_planes(eng, 0, planes)
        s, reps = _align(eng, [0, 0, 0], np.tile(state, (3, 1)))
    ref = ir.optimize([planes], K, ie.cfg([1], None, *depth_range), init_pose=state)
    assert ref["valid_pixels"] == [expected] and ref["iterations"] == [1] and ref["flags"] == 0
    for k in range(3):
        assert list(reps[k].valid_pixels[:1]) == [expected] and list(reps[k].iterations[:1]) == [1] and reps[k].flags == 0
        assert _record(s[k], reps[k], 1) == _record(s[0], reps[0], 1)
    _hold("B", f"{w}x{h} {shift:+.2f} {depth_range}", s[0], reps[0], ref, 1)


# ---- C. Exp's three regimes, from one iteration ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ie.EXP_SEEDS)
def test_inverse_exp_regimes(seed):
    """One iteration from the zero state leaves state_from_pose(Exp(xi)), xi = -lambda H^-1 g: the step length is chosen, from
    the checker's step on the device's planes, so that |omega| is 5e-5 and 9.9e-5 (the Taylor side of the switch at
    |omega|^2 = 1e-8), 1.01e-4, 0.3 and 0.783 (lanes 0 and 1 both in the polynomials), 0.80 and 1.2 (th beyond pi/4, th / 2
    inside), 2.0 and 3.0 (both beyond): Exp, the composition and the three-lane atan2 at angles up to 3 rad."""
    p = ie.exp_pair(seed)
    K = p["K"]
    met, worst = set(), 0.0
    with _engine(K, ie.EXP_W, ie.EXP_H, 2, [1]) as eng:         # the planes do not depend on the step length
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 1, [1])
    for target in ie.EXP_TARGETS:
        step_length, xi = ie.exp_lambda(pyr[0], K, target)
        lam = [step_length]
        with _engine(K, ie.EXP_W, ie.EXP_H, 2, [1], lam=lam) as eng:
            _upload(eng, [p])
            s, reps = _align(eng, [0, 0, 0])
        met.add(ie.exp_regime(xi))
        ref = ir.optimize(pyr, K, ie.cfg([1], lam=lam))
        assert ref["flags"] == 0 and ref["iterations"] == [1]
        worst = max(worst, _hold("C", f"seed {seed} |omega| {target} lambda {lam[0]:.4g}", s[0], reps[0], ref, 1))
        for k in range(3):
            assert _record(s[k], reps[k], 1) == _record(s[0], reps[0], 1)
    assert met == {(True, False, False), (False, False, False), (False, True, False), (False, True, True)}, met
    print(f"part C seed {seed}: largest distance / bar {worst:.3g}")


# ---- D. large angles ---------------------------------------------------------------------------------------------------
def test_inverse_initial_states_in_every_branch():
    """edge_states.initial_states() (branches 2 and 3 of write_pose_constants on each axis, both signs, pi - 0.3 on pitch
    and roll) as one batch of 32, three fixed iterations on each of two levels: 28 stay finite under the flat bar, the four
    with pitch or roll at +-1.2 lose every row."""
    p = ie.angle_pair()
    inits = np.array(edge_states.initial_states())
    n, nl = len(inits), len(ie.ANGLE_MAX_ITER)
    assert n == 32
    with _engine(p["K"], ie.ANGLE_W, ie.ANGLE_H, 2, ie.ANGLE_MAX_ITER) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, nl, ie.ANGLE_MAX_ITER)
        s, reps = _align(eng, [0] * n, inits)
    finite, lost, worst = 0, 0, 0.0
    for i in range(n):
        ref = ir.optimize(pyr, p["K"], ie.cfg(ie.ANGLE_MAX_ITER), init_pose=inits[i])
        worst = max(worst, _hold("D", f"state {i} {inits[i][3:]}", s[i], reps[i], ref, nl))
        if np.all(np.isfinite(ref["state"])):
            finite += 1
            assert np.all(np.isfinite(s[i])) and reps[i].flags == 0
        else:
            lost += 1
            assert ref["valid_pixels"] == [0, 0] and ref["flags"] == BOTH
            assert list(reps[i].valid_pixels[:nl]) == [0, 0] and reps[i].flags == BOTH and np.all(np.isnan(s[i]))
            assert abs(inits[i][3:][np.argmax(np.abs(inits[i][3:]))]) == 1.2
    assert (finite, lost) == (ie.ANGLE_FINITE, ie.ANGLE_LOST) and finite >= 28
    print(f"part D edge states: largest distance / bar {worst:.3g}")


def test_inverse_large_in_plane_motions():
    """True yaw of 0.5, 0.7 and 0.9 rad, started near the truth, ended by the gradient threshold."""
    for p, init in ie.motion_pairs():
        with _engine(p["K"], ie.MOTION_W, ie.MOTION_H, 2, ie.MOTION_MAX_ITER, ie.MOTION_MIN_GRAD) as eng:
            _upload(eng, [p])
            pyr = _device_pyramid(eng, 0, 1, 1, ie.MOTION_MAX_ITER)
            s, reps = _align(eng, [0] * 3, np.tile(init, (3, 1)))
        ref = ir.optimize(pyr, p["K"], ie.cfg(ie.MOTION_MAX_ITER, ie.MOTION_MIN_GRAD), init_pose=init)
        assert 1 < ref["iterations"][0] < ie.MOTION_MAX_ITER[0]
        _hold("D", f"yaw {p['motion'][3]}", s[0], reps[0], ref, 1)
        assert abs(s[0][3] - p["motion"][3]) < 0.05
        for k in range(3):
            assert _record(s[k], reps[k], 1) == _record(s[0], reps[0], 1)


def test_inverse_nonfinite_initial_angle():
    """A NaN and an inf initial yaw among eight healthy pairs: the two report NONFINITE and a NaN pose, as the checker does;
    the other eight keep the bits each has aligned alone."""
    p = ie.angle_pair()
    states, bad = ie.nonfinite_batch()
    nl = len(ie.ANGLE_MAX_ITER)
    with _engine(p["K"], ie.ANGLE_W, ie.ANGLE_H, 2, ie.ANGLE_MAX_ITER) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, nl, ie.ANGLE_MAX_ITER)
        s, reps = _align(eng, [0] * len(states), states)
        for k in range(len(states)):
            if k in bad:
                continue
            s1, reps1 = _align(eng, [0], states[k][None])
            assert _record(s[k], reps[k], nl) == _record(s1[0], reps1[0], nl), k
            assert reps[k].flags == 0
    for k in range(len(states)):
        ref = ir.optimize(pyr, p["K"], ie.cfg(ie.ANGLE_MAX_ITER), init_pose=states[k])
        _hold("D", f"position {k} yaw {states[k][3]}", s[k], reps[k], ref, nl)
        if k in bad:
            assert ref["iterations"] == [1, 1] and ref["flags"] & ir.PAIR_NONFINITE
            assert reps[k].flags & ir.PAIR_NONFINITE and np.all(np.isnan(s[k]))


# ---- E. step length ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", ie.STEP_LAMS, ids=["lam_0.7_0.5", "lam_1.0_0.7"])
def test_inverse_step_length(lam):
    """lambda below 1 and different on the two levels, at fixed iterations and under thresholds: the checker's result under
    lambda = 1 or under the levels' lambdas exchanged is more than a thousand bars away (tests/test_inverse_edges_cpu.py)."""
    small, wide = ie.step_pairs()
    worst = 0.0
    for pairs, w, h, is_wide in ((small, ie.WQ_W, ie.WQ_H, False), ([wide], ie.STEP_WIDE_W, ie.STEP_WIDE_H, True)):
        for name, mi, mg in ie.step_configs(is_wide):
            with _engine(pairs[0]["K"], w, h, 2 * len(pairs), mi, mg, lam=lam) as eng:
                _upload(eng, pairs)
                pyr = [_device_pyramid(eng, 2 * i, 2 * i + 1, 2, mi) for i in range(len(pairs))]
                s, reps = _align(eng, list(range(len(pairs))))
            for i, p in enumerate(pairs):
                ref = ir.optimize(pyr[i], p["K"], ie.cfg(mi, mg, lam=lam))
                assert ref["flags"] == 0
                if name == "threshold":
                    assert all(1 < it < m for it, m in zip(ref["iterations"], mi)), ref["iterations"]
                worst = max(worst, _hold("E", f"{w}x{h} pair {i} {name} lambda {lam}", s[i], reps[i], ref, 2))
    print(f"part E lambda {lam}: largest distance / bar {worst:.3g}")


# ---- F. intrinsics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ie.K_SHIFTS, ids=["ox+_oy-", "ox-_oy+"])
@pytest.mark.parametrize("w,h", ie.K_SIZES, ids=["75x53", "80x60"])
def test_inverse_fy_differs_from_fx(w, h, shift):
    """fy = 1.1 fx, the principal point off the half-integer grid: fx and fy each reach the warp and the row's two
    image-gradient columns where they belong (a row with either focal length in the wrong place ends more than a thousand
    bars away: tests/test_inverse_edges_cpu.py)."""
    p, K = ie.intrinsics_problem(w, h, shift)
    with _engine(K, w, h, 2, ie.K_MAX_ITER) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 2, ie.K_MAX_ITER)
        s, reps = _align(eng, [0, 0, 0], np.tile(ie.K_INIT, (3, 1)))
    ref = ir.optimize(pyr, K, ie.cfg(ie.K_MAX_ITER), init_pose=ie.K_INIT)
    assert ref["flags"] == 0 and min(ref["valid_pixels"]) > 500
    _hold("F", f"{w}x{h} shift {shift}", s[0], reps[0], ref, 2)
    with ie.row_focal_mutant("fy_fx"):
        alt = ir.optimize(pyr, K, ie.cfg(ie.K_MAX_ITER), init_pose=ie.K_INIT)
    assert np.abs(alt["state"] - ref["state"]).max() > 1e3 * ir.pose_bar(ref["cond"], ref["state"])
    for k in range(3):
        assert _record(s[k], reps[k], 2) == _record(s[0], reps[0], 2)


# ---- G. five, six and seven rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ie.ROWS_LAYOUTS)
def test_inverse_systems_of_five_six_and_seven_rows(layout):
    """Exactly 6 rows of real data and 7, well posed (cond(J^T J) about 2e2): flags 0, exact counts and the pose within the
    flat bar after one iteration and after three.  With a constant source (H exactly zero: an exact zero pivot on both
    sides) 5 valid depths report RANK_DEFICIENT | NONFINITE and 6 report NONFINITE alone: the boundary last_valid < 6.  The
    rows sit in one chunk of one wave, or in all four waves (the count and the system are summed across waves)."""
    seed = ie.ROWS_SEED[layout]
    for count, mi in ((6, [1]), (6, [ie.ROWS_ITER]), (7, [1]), (7, [ie.ROWS_ITER])):
        K, planes = ie.rows_problem(seed, layout, count)
        with _engine(K, ie.ROWS_W, ie.ROWS_H, 2, mi) as eng:
            _set_planes(eng, 0, planes)
            s, reps = _align(eng, [0, 0, 0])
        for k in range(3):
            assert _record(s[k], reps[k], 1) == _record(s[0], reps[0], 1)
        ref = ir.optimize([planes], K, ie.cfg(mi))
        assert ref["valid_pixels"] == [count] and ref["flags"] == 0 and ref["iterations"] == mi
        assert list(reps[0].valid_pixels[:1]) == [count] and list(reps[0].iterations[:1]) == mi and reps[0].flags == 0
        _hold("G", f"{layout} {count} rows {mi[0]} iterations", s[0], reps[0], ref, 1)
    for count, flags in ((5, BOTH), (6, ir.PAIR_NONFINITE)):
        K, planes = ie.rows_problem(seed, layout, count, constant_source=True)
        with _engine(K, ie.ROWS_W, ie.ROWS_H, 2, [ie.ROWS_ITER]) as eng:
            _set_planes(eng, 0, planes)
            s, reps = _align(eng, [0, 0, 0])
        ref = ir.optimize([planes], K, ie.cfg([ie.ROWS_ITER]))
        assert ref["flags"] == flags and ref["valid_pixels"] == [count] and ref["iterations"] == [1]
        for k in range(3):
            _hold("G", f"{layout} constant source, {count} rows", s[k], reps[k], ref, 1)
            assert int(reps[k].flags) == flags and np.all(np.isnan(s[k]))


@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_inverse_small_systems_among_healthy_pairs(order):
    """The 6- and 7-row systems and the two constant-source ones between healthy pairs in one enqueue, in both orders: every
    report equals the checker's, and the healthy pairs keep the bits they have alone."""
    healthy = ie.work_queue_pairs()[:ie.WQ_D]
    mi = [ie.ROWS_ITER]
    special = []
    for name, layout, count, const in ie.ROWS_MIXED:
        K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
        assert np.array_equal(K, healthy[0]["K"])
        special.append((name, planes))
    n = len(healthy) + len(special)
    with _engine(healthy[0]["K"], ie.ROWS_W, ie.ROWS_H, 2 * n, mi) as eng:
        _upload(eng, healthy)
        for j, (_, planes) in enumerate(special):
            _set_planes(eng, len(healthy) + j, planes)
        pyr = [_device_pyramid(eng, 2 * i, 2 * i + 1, 1, mi) for i in range(n)]
        which = [3, 0, 4, 1, 5, 2, 6, 0]                        # special and healthy alternate; pair 0 comes back at the end
        if order == "reversed":
            which = which[::-1]
        s, reps = _align(eng, which)
        alone = {i: _align(eng, [i]) for i in range(len(healthy))}
    refs = [ir.optimize(pyr[i], healthy[0]["K"], ie.cfg(mi)) for i in range(n)]
    assert [r["flags"] for r in refs[len(healthy):]] == [0, BOTH, 0, ir.PAIR_NONFINITE]
    assert [r["valid_pixels"] for r in refs[len(healthy):]] == [[6], [5], [7], [6]]
    for k, i in enumerate(which):
        _hold("G", f"{order} position {k} pair {i}", s[k], reps[k], refs[i], 1)
        if i in alone:
            a = alone[i]
            assert _record(s[k], reps[k], 1) == _record(a[0][0], a[1][0], 1), (k, i)
            assert reps[k].flags == 0


# ---- H. a skipped level and a long level ---------------------------------------------------------------------------------
def test_inverse_skipped_level():
    """max_num_iterations [5, 0, 5]: level 1 reports one iteration and the checker's valid_pixels, no launch names it, the
    state level 2 leaves enters level 0, and the result is not that of [5, 5, 5]."""
    p = ie.skip_pair()
    nl = 3
    got = {}
    for mi in (ie.SKIP_MAX_ITER, ie.FULL_MAX_ITER):
        with _engine(p["K"], ie.SKIP_W, ie.SKIP_H, 2, mi) as eng:
            _upload(eng, [p])
            pyr = _device_pyramid(eng, 0, 1, nl, mi)
            s, reps = _align(eng, [0])
            levels = [l["levels"] for l in eng.last_launches()]
        ref = ir.optimize(pyr, p["K"], ie.cfg(mi))
        assert levels == [[l] for l in (2, 1, 0) if mi[l] > 0], levels
        _hold("H", f"max_iter {mi}", s[0], reps[0], ref, nl)
        got[tuple(mi)] = (_bits(s[0]), list(reps[0].iterations[:nl]), list(reps[0].valid_pixels[:nl]), ref)
    skip, full = got[tuple(ie.SKIP_MAX_ITER)], got[tuple(ie.FULL_MAX_ITER)]
    assert skip[1] == [5, 1, 5] and skip[2][1] == skip[3]["valid_pixels"][1] == 0 and full[1] == [5, 5, 5]
    assert skip[0] != full[0]
    assert np.abs(skip[3]["state"] - full[3]["state"]).max() > 1e3 * ir.pose_bar(full[3]["cond"], full[3]["state"])


def test_inverse_long_level():
    """One 80x60 level at 50 fixed iterations, the benchmark's count: 50 compositions of (R, t) without re-orthonormalising
    stay within the flat bar of the checker (whose own |R^T R - I| ends below 1e-13: tests/test_inverse_edges_cpu.py)."""
    p = ie.long_pair()
    mi = [ie.LONG_ITER]
    with _engine(p["K"], ie.LONG_W, ie.LONG_H, 2, mi) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        s, reps = _align(eng, [0, 0, 0])
    ref, R = ie.final_rotation(pyr, p["K"], ie.cfg(mi))
    assert ref["iterations"] == mi and ref["flags"] == 0 and np.abs(R.T @ R - np.eye(3)).max() < ie.ORTHONORMAL_BELOW
    _hold("H", f"{ie.LONG_ITER} iterations", s[0], reps[0], ref, 1)
    for k in range(3):
        assert _record(s[k], reps[k], 1) == _record(s[0], reps[0], 1)
