"""The affine-illumination kernel (gn_affine_kernel.hip) where tests/test_gpu_affine.py does not reach: the
second trip of its persistent loop and the eight-queue draw, rows and clamped taps at exact positions and depth exactly at
the gate, initial states in every branch of the device's sin / cos, degenerate pairs beside healthy ones in one launch, a
skipped level between two that run; step lengths other than 1 that differ between the levels, fy != fx with a principal
point off the half-integer grid, and well-posed systems of exactly 8 and 9 rows beside one of 7.  The reference of every comparison is tests/affine_ref.py in fp64 on the planes as the
device holds them; the bars are test_gpu_affine._compare's (iterations, valid_pixels and flags exact, state and gradient
norm to affine_ref.pose_bar).  Every fixture (tests/affine_edges.py) is chosen to hold the flat bar and to stay clear of its
gradient thresholds; tests/test_affine_edges_cpu.py asserts both without a device."""
import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

import affine_edges as ae
import affine_ref as ar
import edge_states
# (helpers of the first affine GPU file, used as they are so that both files hold the device to the same bars)
from test_gpu_affine import AFFINE, MARGIN_FLOOR, _bits, _compare, _device_pyramid

assert ae.MARGIN_FLOOR == MARGIN_FLOOR

pytestmark = pytest.mark.gpu


def _engine(K, w, h, frames, mi, mg=None, depth_range=None, lam=None):
    nl = len(mi)
    eng = odometry.AlignmentEngine()
    eng.set_config(native.make_config(num_levels=nl, max_iter=mi, min_grad=mg if mg else [0.0] * nl, lam=lam))
    eng.set_objective(AFFINE)
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


def _align(eng, which, inits=None):
    """Pairs which[k] of _upload in one enqueue -> per position (pose bits, (alpha, beta) bits, report), and the arrays."""
    which = np.asarray(which, dtype=int)
    s, reps = eng.align_pairs(2 * which, 2 * which + 1, init_states=inits, want_reports=True)
    ab = eng.fetch_illumination(len(which))
    assert {l["kind"] for l in eng.last_launches()} == {"affine"}
    return s, ab, reps


def _record(s, ab, rep, nl):
    """Everything a pair reports, for bit-for-bit comparison."""
    return (_bits(s), _bits(ab), list(rep.iterations[:nl]), list(rep.valid_pixels[:nl]), int(rep.flags),
            _bits([rep.gradient_norm]))


def _hold(part, what, s, ab, rep, ref, nl, expect_flat=True):
    """test_gpu_affine._compare, and the distance / bar of the pair printed for DESIGN.md §14's table."""
    _compare(s, ab, rep, ref, nl, expect_flat=expect_flat)
    if np.all(np.isfinite(ref["state"])):
        ratio = np.abs(np.concatenate([s, ab]) - ref["state"]).max() / ar.pose_bar(ref["cond"], ref["state"])
        print(f"part {part} {what}: distance / bar {ratio:.3f}")


# ---- A. more pairs than resident workgroups ----------------------------------------------------------------------------
def test_affine_work_queue():
    """N = 3 G + 5 pairs (G: the persistent grid of a large enqueue) drawn from four tiny pairs, one of them with an all-NaN
    source depth: every workgroup takes several trips through the kernel's pair loop, from eight queues.  Every position
    equals, bit for bit, the same pair aligned alone -- a flag, a gain, an offset or a prefetched value that survived from
    one pair to the next on a workgroup would break that somewhere -- on three enqueues in a row (both slots reused: the
    (alpha, beta) buffer is cleared), and a second list starts every pair from its own non-zero state."""
    nl = ae.WQ_LEVELS
    pairs = ae.work_queue_pairs()
    K = pairs[0]["K"]
    cfg = ae.cfg(ae.WQ_MAX_ITER, ae.WQ_MIN_GRAD)
    with _engine(K, ae.WQ_W, ae.WQ_H, 8, ae.WQ_MAX_ITER, ae.WQ_MIN_GRAD) as eng:
        _upload(eng, pairs)
        pyr = [_device_pyramid(eng, 2 * i, 2 * i + 1, nl, ae.WQ_MAX_ITER) for i in range(4)]
        alone = []
        for i in range(4):                                      # the 1-pair probes: held to the checker
            s, ab, reps = _align(eng, [i])
            assert eng.last_launches()[0]["workgroups"] == 1
            ref = ar.optimize(pyr[i], K, cfg)
            _hold("A", f"pair {i}", s[0], ab[0], reps[0], ref, nl)
            alone.append(_record(s[0], ab[0], reps[0], nl))
        assert alone[ae.WQ_D][3:5] == ([0, 0], ar.PAIR_RANK_DEFICIENT | ar.PAIR_NONFINITE)
        assert len({repr(a) for a in alone}) == 4
        _align(eng, [0] * 4096)
        G = eng.last_launches()[0]["workgroups"]
        N = 3 * G + 5
        which = ae.work_queue_list(N)
        assert set(which.tolist()) == {0, 1, 2, 3}
        for run in range(3):
            s, ab, reps = _align(eng, which)
            launches = eng.last_launches()
            print(f"run {run}: N = {N}, grid {launches[0]['workgroups']} (G = {G})")
            assert len(launches) == nl and all(l["workgroups"] == G < N for l in launches) and N >= 512
            for k in range(N):
                assert _record(s[k], ab[k], reps[k], nl) == alone[which[k]], (run, k, which[k])

        # every pair from its own non-zero state: states[pair] is read per pair inside the loop
        N2 = 520
        states, pick = ae.work_queue_inits(N2)
        which2 = ae.work_queue_list(N2, seed=2)
        combos = sorted({(int(a), int(b)) for a, b in zip(which2, pick)})
        alone2 = {}
        for a, b in combos:
            s, ab, reps = _align(eng, [a], states[b][None])
            ref = ar.optimize(pyr[a], K, cfg, init_pose=states[b])
            _hold("A", f"pair {a} from state {b}", s[0], ab[0], reps[0], ref, nl)
            alone2[(a, b)] = _record(s[0], ab[0], reps[0], nl)
        s, ab, reps = _align(eng, which2, states[pick])
        assert N2 >= 512 and eng.last_launches()[0]["workgroups"] < N2      # eight queues, a second trip somewhere
        for k in range(N2):
            assert _record(s[k], ab[k], reps[k], nl) == alone2[(int(which2[k]), int(pick[k]))], (k, which2[k], pick[k])
        assert len({repr(v) for (a, b), v in alone2.items() if a != ae.WQ_D}) == len([c for c in combos if c[0] != ae.WQ_D])


# ---- B. exact positions ------------------------------------------------------------------------------------------------
EXACT_CASES = [(w, h, s, r) for (w, h), shifts in ae.EXACT_SIZES.items() for s in shifts for r in ae.RANGES]


@pytest.mark.parametrize("w,h,shift,depth_range", EXACT_CASES,
                         ids=[f"{w}x{h}_{s:+.2f}_{r[0]}_{r[1]}" for w, h, s, r in EXACT_CASES])
def test_affine_exact_rows_and_taps(w, h, shift, depth_range):
    """Every projected coordinate is exactly c + shift, r + shift: at +-0.5 the outermost column and row sit on -0.5 /
    W - 0.5 and are out (both comparisons are strict), at +-0.25 they are rows whose taps are clamped, at +-0.75 they are
    out; a column at min_depth and a row at max_depth are out (for the range 0.5 / 2.0 also depths 0.4 and 3.0)."""
    K, planes, state = ae.exact_problem(w, h, shift, depth_range)
    i0, d0, i1, gx, gy = planes
    expected = ae.exact_rows(d0, shift)
    with _engine(K, w, h, 2, [1], depth_range=depth_range) as eng:
        eng.set_level_planes(0, 0, intensity=i0, depth=d0)
        eng.set_level_planes(1, 0, intensity=i1, grad_x=gx, grad_y=gy)
        s, ab, reps = _align(eng, [0, 0, 0], np.tile(state, (3, 1)))
    ref = ar.optimize([planes], K, ae.cfg([1], None, *depth_range), init_pose=state)
    assert ref["valid_pixels"] == [expected] and ref["iterations"] == [1] and ref["flags"] == 0
    for k in range(3):
        assert list(reps[k].valid_pixels[:1]) == [expected] and list(reps[k].iterations[:1]) == [1] and reps[k].flags == 0
        assert _record(s[k], ab[k], reps[k], 1) == _record(s[0], ab[0], reps[0], 1)
    _hold("B", f"{w}x{h} {shift:+.2f} {depth_range}", s[0], ab[0], reps[0], ref, 1)


# ---- C. large angles ---------------------------------------------------------------------------------------------------
def test_affine_initial_states_in_every_branch():
    """edge_states.initial_states() (branches 2 and 3 of write_pose_constants on each axis, both signs, pi - 0.3 on pitch
    and roll) as one batch, three fixed iterations on each of two levels.  Many of these starts see few rows or none:
    rows, flags and the iteration at which a state stops being finite equal the checker's."""
    p = ae.angle_pair()
    inits = np.array(edge_states.initial_states())
    n, nl = len(inits), len(ae.ANGLE_MAX_ITER)
    with _engine(p["K"], ae.ANGLE_W, ae.ANGLE_H, 2, ae.ANGLE_MAX_ITER) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, nl, ae.ANGLE_MAX_ITER)
        s, ab, reps = _align(eng, [0] * n, inits)
    classes, good = dict(flat=0, conditioned=0, nonfinite=0), set()
    for i in range(n):
        ref = ar.optimize(pyr, p["K"], ae.cfg(ae.ANGLE_MAX_ITER), init_pose=inits[i])
        finite = bool(np.all(np.isfinite(ref["state"])))
        is_flat = finite and bool(ref["cond"] <= 1e5)
        classes["flat" if is_flat else "conditioned" if finite else "nonfinite"] += 1
        if is_flat and min(ref["valid_pixels"]) > 100:
            good.add(ae.angle_label(inits[i]))
        _hold("C", f"state {i} {ae.angle_label(inits[i])}", s[i], ab[i], reps[i], ref, nl, expect_flat=is_flat)
    # on the planes the device holds, as on the CPU pyramid (test_affine_edges_cpu.py): every axis, sign and branch keeps a
    # pair under the flat bar with more than 100 rows on both levels
    assert good == {(axis, sign, branch) for axis in range(3) for sign in (1, -1) for branch in (2, 3)}, good
    assert classes == dict(flat=28, conditioned=0, nonfinite=4), classes


def test_affine_large_in_plane_motions():
    """True yaw of 0.5, 0.7 and 0.9 rad (branches 2, 2, 3), started near the truth, ended by the gradient threshold."""
    for p, init in ae.motion_pairs():
        with _engine(p["K"], ae.MOTION_W, ae.MOTION_H, 2, ae.MOTION_MAX_ITER, ae.MOTION_MIN_GRAD) as eng:
            _upload(eng, [p])
            pyr = _device_pyramid(eng, 0, 1, 1, ae.MOTION_MAX_ITER)
            s, ab, reps = _align(eng, [0] * 3, np.tile(init, (3, 1)))
        ref = ar.optimize(pyr, p["K"], ae.cfg(ae.MOTION_MAX_ITER, ae.MOTION_MIN_GRAD), init_pose=init)
        assert ref["iterations"][0] < ae.MOTION_MAX_ITER[0] and abs(ref["state"][3] - p["motion"][3]) < 0.05
        _hold("C", f"yaw {p['motion'][3]}", s[0], ab[0], reps[0], ref, 1)
        for k in range(3):
            assert _record(s[k], ab[k], reps[k], 1) == _record(s[0], ab[0], reps[0], 1)


def test_affine_nonfinite_initial_angle():
    """A NaN and an inf initial yaw among eight healthy pairs: the healthy ones keep the bits of the batch without them,
    the two report what the checker does (no row, NONFINITE after one iteration on every level)."""
    p = ae.angle_pair()
    states, bad = ae.nonfinite_batch()
    good = [k for k in range(len(states)) if k not in bad]
    nl = len(ae.ANGLE_MAX_ITER)
    with _engine(p["K"], ae.ANGLE_W, ae.ANGLE_H, 2, ae.ANGLE_MAX_ITER) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, nl, ae.ANGLE_MAX_ITER)
        s, ab, reps = _align(eng, [0] * len(states), states)
        s2, ab2, reps2 = _align(eng, [0] * len(good), states[good])
    for j, k in enumerate(good):
        assert _record(s[k], ab[k], reps[k], nl) == _record(s2[j], ab2[j], reps2[j], nl), k
        assert reps[k].flags == 0
    _hold("C", "healthy beside NaN / inf", s[0], ab[0], reps[0],
          ar.optimize(pyr, p["K"], ae.cfg(ae.ANGLE_MAX_ITER), init_pose=states[0]), nl)
    for k in bad:
        ref = ar.optimize(pyr, p["K"], ae.cfg(ae.ANGLE_MAX_ITER), init_pose=states[k])
        assert ref["iterations"] == [1, 1] and ref["flags"] & ar.PAIR_NONFINITE
        _hold("C", f"bad yaw {states[k][3]}", s[k], ab[k], reps[k], ref, nl)


# ---- D. mixed batch, skipped level -------------------------------------------------------------------------------------
def _mixed_engine(pairs, kinds, mi):
    eng = _engine(pairs[kinds[0]]["K"], ae.MIX_W, ae.MIX_H, 2 * len(kinds), mi)
    _upload(eng, [pairs[k] for k in kinds])
    for i, k in enumerate(kinds):
        for l, d in enumerate(pairs[k].get("sparse", [])):
            if mi[l] > 0:
                eng.set_level_planes(2 * i, l, depth=d)
    return eng


@pytest.mark.parametrize("mi", [ae.MIX_MAX_ITER, [0, 0, 4]], ids=["three_levels", "coarsest_only"])
def test_affine_mixed_batch(mi):
    """Healthy pairs, a black source (exact zero pivot), an all-NaN depth, and black sources with exactly 7 and exactly 8
    valid depths on every level, in one enqueue of 12: every report equals the checker's, the healthy pairs keep the bits
    they have alone.  With only the coarsest level run, the pair with 8 rows stays clear of RANK_DEFICIENT (on three levels
    the NaN state it leaves sees no row on the next one, which sets the flag on both sides)."""
    pairs = ae.mixed_pairs()
    kinds = list(ae.MIX_SEEDS)
    nl = ae.MIX_LEVELS
    which = [kinds.index(k) for k in ae.MIX_KINDS]
    with _mixed_engine(pairs, kinds, mi) as eng:
        pyr = [_device_pyramid(eng, 2 * i, 2 * i + 1, nl, mi) for i in range(len(kinds))]
        s, ab, reps = _align(eng, which)
        alone = {i: _align(eng, [i]) for i in set(which) if kinds[i].startswith("healthy")}
    assert len(which) == 12 and len(alone) == 3
    refs = [ar.optimize(pyr[i], pairs[k]["K"], ae.cfg(mi)) for i, k in enumerate(kinds)]
    for k, i in enumerate(which):
        _hold("D", f"position {k} {kinds[i]}", s[k], ab[k], reps[k], refs[i], nl)
        if i in alone:
            a = alone[i]
            assert _record(s[k], ab[k], reps[k], nl) == _record(a[0][0], a[1][0], a[2][0], nl), (k, kinds[i])
            assert reps[k].flags == 0
    both = ar.PAIR_RANK_DEFICIENT | ar.PAIR_NONFINITE
    enough = both if sum(m > 0 for m in mi) > 1 else ar.PAIR_NONFINITE      # NP rows or more on the only level run
    expect = dict(black=enough, nan_depth=both, seven=both, eight=enough)
    for kind, flags in expect.items():
        i = kinds.index(kind)
        assert refs[i]["flags"] == flags, (kind, refs[i]["flags"])
    assert refs[kinds.index("seven")]["valid_pixels"][2] == 7 and refs[kinds.index("eight")]["valid_pixels"][2] == 8


def test_affine_skipped_level():
    """max_num_iterations [5, 0, 5] under an exposure change: level 1 reports one iteration and no launch names it, the
    state level 2 leaves -- alpha and beta with it -- enters level 0, and the result is not that of [5, 5, 5]."""
    p = ae.exposure_pair()
    nl = 3
    got = {}
    for mi in (ae.SKIP_MAX_ITER, ae.FULL_MAX_ITER):
        with _engine(p["K"], ae.SKIP_W, ae.SKIP_H, 2, mi) as eng:
            _upload(eng, [p])
            pyr = _device_pyramid(eng, 0, 1, nl, mi)
            s, ab, reps = _align(eng, [0])
            levels = [l["levels"] for l in eng.last_launches()]
        ref = ar.optimize(pyr, p["K"], ae.cfg(mi))
        assert levels == [[l] for l in (2, 1, 0) if mi[l] > 0], levels
        _hold("D", f"max_iter {mi}", s[0], ab[0], reps[0], ref, nl)
        assert np.all(np.abs(ref["state"][6:]) > 1e-3)          # a gain and an offset were carried
        got[tuple(mi)] = (_bits(ab[0]), list(reps[0].iterations[:nl]))
    assert got[tuple(ae.SKIP_MAX_ITER)][1] == [5, 1, 5]
    assert got[tuple(ae.SKIP_MAX_ITER)][0] != got[tuple(ae.FULL_MAX_ITER)][0]


# ---- E. step length ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", ae.STEP_LAMS, ids=["lam_0.7_0.5", "lam_1.0_0.7"])
def test_affine_step_length(lam):
    """lambda below 1 and different on the two levels, at fixed iterations and under thresholds: the checker's result under
    lambda = 1 or under the levels' lambdas exchanged is more than a thousand bars away (tests/test_affine_edges_cpu.py)."""
    small, wide = ae.step_pairs()
    for pairs, w, h, is_wide in ((small, ae.WQ_W, ae.WQ_H, False), ([wide], ae.STEP_WIDE_W, ae.STEP_WIDE_H, True)):
        for name, mi, mg in ae.step_configs(is_wide):
            with _engine(pairs[0]["K"], w, h, 2 * len(pairs), mi, mg, lam=lam) as eng:
                _upload(eng, pairs)
                pyr = [_device_pyramid(eng, 2 * i, 2 * i + 1, 2, mi) for i in range(len(pairs))]
                s, ab, reps = _align(eng, list(range(len(pairs))))
            for i, p in enumerate(pairs):
                ref = ar.optimize(pyr[i], p["K"], ae.cfg(mi, mg, lam=lam))
                assert ref["flags"] == 0
                _hold("E", f"{w}x{h} pair {i} {name} lambda {lam}", s[i], ab[i], reps[i], ref, 2)


# ---- F. intrinsics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ae.K_SHIFTS, ids=["ox+_oy-", "ox-_oy+"])
@pytest.mark.parametrize("w,h", ae.K_SIZES, ids=["75x53", "80x60"])
def test_affine_fy_differs_from_fx(w, h, shift):
    """fy = 1.1 fx, the principal point off the half-integer grid: fx, fy, 1 / fx, 1 / fy, ox and oy each reach the warp and
    the Jacobian where they belong (the checker with fy := fx differs in state and rows)."""
    p, K = ae.intrinsics_problem(w, h, shift)
    with _engine(K, w, h, 2, ae.K_MAX_ITER) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 2, ae.K_MAX_ITER)
        s, ab, reps = _align(eng, [0, 0, 0], np.tile(ae.K_INIT, (3, 1)))
    ref = ar.optimize(pyr, K, ae.cfg(ae.K_MAX_ITER), init_pose=ae.K_INIT)
    alt = ar.optimize(pyr, ae.with_fy_equal_fx(K), ae.cfg(ae.K_MAX_ITER), init_pose=ae.K_INIT)
    assert alt["valid_pixels"] != ref["valid_pixels"] and ref["flags"] == 0
    _hold("F", f"{w}x{h} shift {shift}", s[0], ab[0], reps[0], ref, 2)
    for k in range(3):
        assert _record(s[k], ab[k], reps[k], 2) == _record(s[0], ab[0], reps[0], 2)


# ---- G. 7, 8 and 9 rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ae.ROWS_LAYOUTS)
def test_affine_well_posed_systems_of_eight_and_nine_rows(layout):
    """Exactly NP rows of real data, well posed (cond(J^T J) 4e3 ... 5e3): flags 0 and the state within the flat bar after
    one iteration and after three; nine rows alike; with seven the pair is RANK_DEFICIENT after its one iteration (its step
    is rounding noise on either side: nothing is asserted on the state).  The rows sit in one chunk of one wave, or in all
    four waves."""
    seed = ae.ROWS_SEED[layout]
    for count, mi in ((8, [1]), (8, [ae.ROWS_ITER]), (9, [1]), (9, [ae.ROWS_ITER]), (7, [1])):
        K, planes = ae.rows_problem(seed, layout, count)
        i0, d0, i1, gx, gy = planes
        with _engine(K, ae.ROWS_W, ae.ROWS_H, 2, mi) as eng:
            eng.set_level_planes(0, 0, intensity=i0, depth=d0)
            eng.set_level_planes(1, 0, intensity=i1, grad_x=gx, grad_y=gy)
            s, ab, reps = _align(eng, [0, 0, 0])
        for k in range(3):
            assert _record(s[k], ab[k], reps[k], 1) == _record(s[0], ab[0], reps[0], 1)
        assert list(reps[0].valid_pixels[:1]) == [count] and list(reps[0].iterations[:1]) == mi
        if count == 7:
            assert reps[0].flags & ar.PAIR_RANK_DEFICIENT
            continue
        ref = ar.optimize([planes], K, ae.cfg(mi))
        assert ref["valid_pixels"] == [count] and ref["flags"] == 0 and reps[0].flags == 0
        _hold("G", f"{layout} {count} rows {mi[0]} iterations", s[0], ab[0], reps[0], ref, 1)
