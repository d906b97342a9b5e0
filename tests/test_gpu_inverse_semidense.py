"""GPU tests of the semi-dense inverse-compositional objective (PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) against
its CPU checker (tests/semidense_ref.py: objective 5's checker on a source whose depth is NaN off the selection).  The
checker is fed the planes exactly as the device holds them, and every fixture passes semidense_cases.precheck on THOSE planes
first: no pixel within 1e-12 relative of the threshold, cond(J^T J) <= 1e5, no iteration within 1e-6 of its gradient
threshold, output angles clear of the cuts.  Bars: test_gpu_inverse._compare's (iterations, rows and flags exact, the pose
within pose_bar, gradient_norm to 1e-9 relative), and `selected` exact."""
import ctypes as C
import os

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, synthetic

import inverse_ref as ir
import semidense_cases as sc
import semidense_ref as sr
from test_gpu_inverse import MARGIN_FLOOR, _bits, _compare, _device_pyramid, _status

assert sc.MARGIN_FLOOR == MARGIN_FLOOR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "config_files")
SEMI = native.OBJECTIVE_INVERSE_SEMIDENSE
INVERSE = native.OBJECTIVE_INVERSE_COMPOSITIONAL


def _engine(K, w, h, frames, mi, mg=None, tau=None, depth_range=None):
    nl = len(mi)
    eng = odometry.AlignmentEngine()
    eng.set_config(native.make_config(num_levels=nl, max_iter=mi, min_grad=mg if mg else [0.0] * nl))
    eng.set_objective(SEMI)
    eng.set_intrinsic_matrix(K)
    if depth_range is not None:
        eng.set_depth_range(*depth_range)
    if tau is not None:
        eng.set_semidense_options(native.make_semidense_options(tau))
    eng.reserve_frames(frames, w, h)
    return eng


def _upload(eng, pairs):
    """Pair i: source frame 2 i, target frame 2 i + 1."""
    for i, p in enumerate(pairs):
        eng.upload_frame(2 * i, p["gray0"], p["depth0"])
        eng.upload_frame(2 * i + 1, p["gray1"], p["depth1"])


def _set_planes(eng, i, planes):
    i0, d0, gx0, gy0, i1 = planes
    eng.set_level_planes(2 * i, 0, intensity=i0, depth=d0, grad_x=gx0, grad_y=gy0)
    eng.set_level_planes(2 * i + 1, 0, intensity=i1)


def _align(eng, which, inits=None):
    """Pairs which[k] in one enqueue -> (states, reports, selected[n, levels]); every launch is this objective's."""
    which = np.asarray(which, dtype=int)
    s, reps = eng.align_pairs(2 * which, 2 * which + 1, init_states=inits, want_reports=True)
    launches = eng.last_launches()
    assert launches and {l["kind"] for l in launches} == {"inverse_semidense"}
    return s, reps, eng.fetch_semidense_reports(len(which))["selected"]


def _record(s, rep, sel, nl):
    """Everything a pair reports, for bit-for-bit comparison."""
    return (_bits(s), list(rep.iterations[:nl]), list(rep.valid_pixels[:nl]), int(rep.flags), _bits([rep.gradient_norm]),
            [int(v) for v in sel[:nl]])


def _hold(s, rep, sel, ref, nl, flat=True):
    print(f"selected {list(sel[:nl])}; checker {ref['selected']}")
    assert [int(v) for v in sel[:nl]] == ref["selected"]
    assert all(int(v) == 0 for v in sel[nl:])
    _compare(s, rep, ref, nl, expect_flat=flat)


def _taus(eng, frame, fraction, nl):
    return odometry.semidense_thresholds(eng, frame, fraction)[:nl]


# ---- 1. parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", sc.PARITY_SIZES)
@pytest.mark.parametrize("fraction", sc.FRACTIONS)
def test_single_level_matches_the_checker(w, h, fraction):
    """test_gpu_inverse's sizes with tau at the device planes' own quantile.  The two strips end with a NaN pose on both
    sides, as under objective 5 (no gradient across: an exactly zero column).  A tenth of 7 x 5 is 4 pixels -- fewer than
    six rows, a system that is singular up to rounding and whose pose is defined on neither side -- so that case runs ONE
    iteration and is held to the counts and the rank flag of that first system."""
    p = sc.parity_pair(w, h)
    healthy = sc.parity_is_healthy(w, h, fraction)
    few = (w, h) == (7, 5) and fraction == 0.1
    mi = [1] if few else [5]
    with _engine(p["K"], w, h, 2, mi) as eng:
        _upload(eng, [p])
        tau = _taus(eng, 0, fraction, 1)
        eng.set_semidense_options(native.make_semidense_options(tau))
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        ref = sc.precheck(pyr, p["K"], sc.cfg(mi), tau, healthy=healthy)
        s, reps, sel = _align(eng, [0])
    if few:
        assert ref["selected"] == [4] and list(sel[0][:1]) == [4] and list(reps[0].valid_pixels[:1]) == ref["valid_pixels"]
        assert list(reps[0].iterations[:1]) == [1] and reps[0].flags & ir.PAIR_RANK_DEFICIENT
        return
    _hold(s[0], reps[0], sel[0], ref, 1)


@pytest.mark.parametrize("yaw", [False, True])
@pytest.mark.parametrize("fraction", sc.FRACTIONS)
def test_three_levels_carry_the_pose(yaw, fraction):
    p, init = sc.carry_pair(yaw)
    nl, mi = 3, [10, 10, 10]
    with _engine(p["K"], 160, 120, 2, mi) as eng:
        _upload(eng, [p])
        tau = _taus(eng, 0, fraction, nl)
        eng.set_semidense_options(native.make_semidense_options(tau))
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        ref = sc.precheck(pyr, p["K"], sc.cfg(mi), tau, init)
        s, reps, sel = _align(eng, [0], None if init is None else init[None])
    _hold(s[0], reps[0], sel[0], ref, nl)
    n = [160 * 120, 80 * 60, 40 * 30]
    assert all(abs(ref["selected"][L] / n[L] - fraction) < 0.05 for L in range(nl))
    if yaw:
        assert abs(s[0][3] - 0.4) < 0.05


def test_vga_pair_with_the_shipped_4_level_file():
    n = native.read_config_file(os.path.join(CFG_DIR, "config_4_level_optimization_analytic.yml"))
    nl = n.num_levels
    mi, mg = list(n.max_num_iterations[:nl]), list(n.min_gradient_norm[:nl])
    p = synthetic.make_pair(21, 640, 480, holes=0.02)
    with _engine(p["K"], 640, 480, 2, mi, mg) as eng:
        _upload(eng, [p])
        tau = _taus(eng, 0, 0.25, nl)
        eng.set_semidense_options(native.make_semidense_options(tau))
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        ref = sc.precheck(pyr, p["K"], sc.cfg(mi, mg), tau)
        s, reps, sel = _align(eng, [0])
    _hold(s[0], reps[0], sel[0], ref, nl)


# ---- 2. tau = 0 ------------------------------------------------------------------------------------------------------
def test_tau_zero_is_objective_5_on_the_same_rows():
    p = synthetic.make_pair(5, 80, 60, holes=0.02)
    nl, mi, mg = 2, [6, 6], [5.0, 5.0]
    with _engine(p["K"], 80, 60, 2, mi, mg) as eng:
        _upload(eng, [p])
        assert list(eng.get_semidense_options().min_pixel_gradient) == [0.0] * native.MAX_LEVELS
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        s7, r7, sel = _align(eng, [0])
        eng.set_objective(INVERSE)
        s5, r5 = eng.align_pairs([0], [1], want_reports=True)
    for L in range(nl):
        d = pyr[L][1]
        assert int(sel[0][L]) == int(((d > 0.3) & (d < 5.0)).sum())
    assert list(r7[0].valid_pixels[:nl]) == list(r5[0].valid_pixels[:nl])
    assert list(r7[0].iterations[:nl]) == list(r5[0].iterations[:nl]) and int(r7[0].flags) == int(r5[0].flags) == 0
    ref = sr.optimize(pyr, p["K"], sc.cfg(mi, mg), [0.0] * nl)
    bar = sr.pose_bar(ref["cond"], ref["state"])
    err = np.abs(s7[0] - s5[0]).max()
    print(f"max |objective 7 - objective 5| = {err:.3e}, bar {bar:.1e}")
    assert err <= bar
    _hold(s7[0], r7[0], sel[0], ref, nl)


# ---- 3. nothing selected ---------------------------------------------------------------------------------------------
def test_nothing_selected():
    """tau = 1e300 (its square is inf): no list, no row, both flags and a NaN state -- for every pair of the enqueue.  And
    at a finite tau under which a flat source selects nothing, the healthy pair beside it has the bits it has alone."""
    pairs = sc.stale_pairs()
    pairs[1] = sc.flat_contrast(pairs[0], 0.1)
    nl, mi = 2, [3, 3]
    with _engine(pairs[0]["K"], sc.STALE_W, sc.STALE_H, 4, mi, tau=1e300) as eng:
        _upload(eng, pairs)
        s, reps, sel = _align(eng, [0, 1, 0])
        for k in range(3):
            assert list(sel[k][:nl]) == [0, 0] and list(reps[k].valid_pixels[:nl]) == [0, 0]
            assert int(reps[k].flags) == sc.BOTH and np.all(np.isnan(s[k])) and list(reps[k].iterations[:nl]) == [1, 1]
        tau = _taus(eng, 0, 0.9, nl)
        eng.set_semidense_options(native.make_semidense_options(tau))
        alone = _align(eng, [0])
        s, reps, sel = _align(eng, [1, 0, 1, 1, 0])
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        ref = sc.precheck(pyr, pairs[0]["K"], sc.cfg(mi), tau)
    _hold(alone[0][0], alone[1][0], alone[2][0], ref, nl)
    for k in (0, 2, 3):
        assert list(sel[k][:nl]) == [0, 0] and int(reps[k].flags) == sc.BOTH and np.all(np.isnan(s[k]))
    for k in (1, 4):
        assert _record(s[k], reps[k], sel[k], nl) == _record(alone[0][0], alone[1][0], alone[2][0], nl)


# ---- 4. the rule's edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sc.EDGE_KINDS)
def test_the_rules_edges(kind):
    K, planes, tau, expected = sc.edge_problem(kind)
    mi = [3]
    with _engine(K, sc.EDGE_W, sc.EDGE_H, 2, mi, tau=[tau]) as eng:
        _set_planes(eng, 0, planes)
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        ref = sc.precheck(pyr, K, sc.cfg(mi), [tau], exact_pixels=kind in ("at_tau", "below_tau"))
        s, reps, sel = _align(eng, [0])
    assert ref["selected"] == [expected] and int(sel[0][0]) == expected
    _hold(s[0], reps[0], sel[0], ref, 1)


# ---- 5. small lists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sc.SMALL_LAYOUTS)
@pytest.mark.parametrize("count", [5, 6, 7])
def test_small_lists(layout, count):
    K, planes = sc.small_problem(layout, count)
    mi = [1] if count == 5 else [sc.SMALL_ITER]
    with _engine(K, sc.SMALL_W, sc.SMALL_H, 2, mi, tau=[sc.TAU]) as eng:
        _set_planes(eng, 0, planes)
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        ref = sc.precheck(pyr, K, sc.cfg(mi), [sc.TAU], healthy=count > 5)
        s, reps, sel = _align(eng, [0])
    assert ref["selected"] == [count] and int(sel[0][0]) == count and list(reps[0].valid_pixels[:1]) == [count]
    if count == 5:              # five rows: singular up to rounding, the pose is defined on neither side
        assert reps[0].flags & ir.PAIR_RANK_DEFICIENT and list(reps[0].iterations[:1]) == [1]
        return
    _hold(s[0], reps[0], sel[0], ref, 1)


@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_small_lists_among_healthy_pairs(order):
    """The lists of 5, 6 and 7 pixels in both layouts between healthy pairs (about half of the pixels selected) in one
    enqueue: every position has the bits of that pair aligned alone."""
    mi = [sc.SMALL_ITER]
    specials = [sc.small_problem(layout, count)[1] for layout in sc.SMALL_LAYOUTS for count in (5, 6, 7)]
    K, healthy = sc.direct_problem(sc.SMALL_W, sc.SMALL_H, 3, list(range(0, sc.SMALL_W * sc.SMALL_H, 2)))
    frames = [healthy] + specials
    with _engine(K, sc.SMALL_W, sc.SMALL_H, 2 * len(frames), mi, tau=[sc.TAU]) as eng:
        for i, planes in enumerate(frames):
            _set_planes(eng, i, planes)
        alone = []
        for i in range(len(frames)):
            s, reps, sel = _align(eng, [i])
            alone.append(_record(s[0], reps[0], sel[0], 1))
        assert alone[0][5] == [sc.SMALL_W * sc.SMALL_H // 2] and alone[0][3] == 0
        assert [a[5][0] for a in alone[1:]] == [5, 6, 7, 5, 6, 7]
        which = []
        for i in range(1, len(frames)):
            which += [0, i]
        which += [0]
        if order == "reversed":
            which = which[::-1]
        s, reps, sel = _align(eng, which)
        for k, i in enumerate(which):
            assert _record(s[k], reps[k], sel[k], 1) == alone[i], (k, i)


# ---- 6. the compact walk ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", sc.WALK_COUNTS)
def test_the_compact_walk(count):
    """All selected pixels in wave 0's chunks (the three other waves have count 0); 63, 64, 65, 128 and 129 records are one,
    one, two, two and three compact chunks: both parities of the two-chunk pipeline and its tail."""
    K, planes = sc.walk_problem(count)
    mi = [sc.WALK_ITER]
    with _engine(K, sc.WALK_W, sc.WALK_H, 2, mi, tau=[sc.TAU]) as eng:
        _set_planes(eng, 0, planes)
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        ref = sc.precheck(pyr, K, sc.cfg(mi), [sc.TAU])
        s, reps, sel = _align(eng, [0])
    assert ref["selected"] == [count]
    _hold(s[0], reps[0], sel[0], ref, 1)


# ---- 7. stale slab ---------------------------------------------------------------------------------------------------
def test_a_short_list_behind_a_long_one():
    """N = 3 G + 5 pairs (G: the persistent grid of a large enqueue) alternating between a source that selects about 90 %
    of its pixels and one that selects about 2 %, on two levels of different size (the slab is sized by level 0): on
    every workgroup a short list follows a long one, whose records still lie in the slab behind the new counts.  Every
    position has the bits of that pair aligned alone -- in three enqueues in a row, and with two enqueues in flight (each
    slot's own workspace) -- and both solo runs are held to the checker."""
    pairs = sc.stale_pairs()
    K = pairs[0]["K"]
    nl, mi = len(sc.STALE_ITER), sc.STALE_ITER
    with _engine(K, sc.STALE_W, sc.STALE_H, 4, mi) as eng:
        _upload(eng, pairs)
        tau = _taus(eng, 0, 0.9, nl)
        eng.set_semidense_options(native.make_semidense_options(tau))
        alone = []
        for i in range(2):
            pyr = _device_pyramid(eng, 2 * i, 2 * i + 1, nl, mi)
            ref = sc.precheck(pyr, K, sc.cfg(mi), tau)
            s, reps, sel = _align(eng, [i])
            assert all(l["workgroups"] == 1 for l in eng.last_launches())
            _hold(s[0], reps[0], sel[0], ref, nl)
            alone.append(_record(s[0], reps[0], sel[0], nl))
        n0 = sc.STALE_W * sc.STALE_H
        assert alone[0][5][0] > 0.8 * n0 and 6 <= alone[1][5][0] < 0.03 * n0
        _align(eng, [0] * 4096)
        G = eng.last_launches()[0]["workgroups"]
        N = 3 * G + 5
        which = np.arange(N) % 2                       # long, short, long, ... in queue order
        for run in range(3):
            s, reps, sel = _align(eng, which)
            launches = eng.last_launches()
            assert len(launches) == nl and all(l["workgroups"] == G < N for l in launches)
            for k in range(N):
                assert _record(s[k], reps[k], sel[k], nl) == alone[which[k]], (run, k)
        # two enqueues in flight: both slots' workspaces, the second list starting with the short pair
        which_b = (np.arange(N) + 1) % 2
        tickets = []
        for w in (which, which_b):
            eng.enqueue_align(2 * w, 2 * w + 1)
            tickets.append(eng.last_ticket())
        for w, t in zip((which, which_b), tickets):
            s, reps = eng.fetch(t, N, want_reports=True)
            for k in range(N):
                assert (_bits(s[k]), list(reps[k].iterations[:nl]), list(reps[k].valid_pixels[:nl]), int(reps[k].flags)) == \
                    alone[w[k]][:4], (t, k)
        sel = eng.fetch_semidense_reports(N)["selected"]
        assert all([int(v) for v in sel[k][:nl]] == alone[which_b[k]][5] for k in range(N))


# ---- 8. bit identity -------------------------------------------------------------------------------------------------
def test_batch_position_and_surface_do_not_change_a_bit():
    """One pair alone, at position 37 of 64, through phovo_odometry_optimize (C ABI) and through the Python class."""
    x = synthetic.make_pair(5, 80, 60, holes=0.02)
    y = synthetic.make_pair(6, 80, 60, holes=0.02)
    nl, mi, mg = 2, [6, 6], [5.0, 5.0]
    ncfg = native.make_config(num_levels=nl, max_iter=mi, min_grad=mg)
    src = [1] * 64
    src[37] = 0
    got, sels = [], []
    with _engine(x["K"], 80, 60, 4, mi, mg) as eng:
        _upload(eng, [x, y])
        tau = _taus(eng, 0, 0.25, nl)
        opt = native.make_semidense_options(tau)
        eng.set_semidense_options(opt)
        s, reps, sel = _align(eng, [0])
        got.append(s[0]); sels.append(list(sel[0][:nl]))
        s, reps, sel = _align(eng, src)
        got.append(s[37]); sels.append(list(sel[37][:nl]))
    lib = native.lib()
    h = C.c_void_p()
    native.check(lib.phovo_odometry_create(0, C.byref(h)), "create")
    try:
        native.check(lib.phovo_odometry_set_objective(h, SEMI), "objective")
        native.check(lib.phovo_odometry_set_config(h, C.byref(ncfg)), "config")
        native.check(lib.phovo_odometry_set_semidense_options(h, C.byref(opt)), "options")
        back = native.SemiDenseOptions()
        native.check(lib.phovo_odometry_get_semidense_options(h, C.byref(back)), "options")
        assert list(back.min_pixel_gradient) == list(opt.min_pixel_gradient)
        k = np.ascontiguousarray(x["K"], dtype=np.float64).reshape(9)
        native.check(lib.phovo_odometry_set_intrinsic_matrix(h, k.ctypes.data_as(C.POINTER(C.c_double))), "K")
        g0, d0, g1 = (np.ascontiguousarray(x["gray0"]), np.ascontiguousarray(x["depth0"], dtype=np.float64),
                      np.ascontiguousarray(x["gray1"]))
        rep = native.SemiDenseReport()
        assert lib.phovo_odometry_get_semidense_report(h, C.byref(rep)) == native.E_NOT_READY
        native.check(lib.phovo_odometry_set_source_frame(h, g0.ctypes.data, 80, d0.ctypes.data, 80 * 8, 80, 60), "source")
        native.check(lib.phovo_odometry_set_target_frame(h, g1.ctypes.data, 80, None, 0, 80, 60), "target")
        native.check(lib.phovo_odometry_optimize(h), "optimize")
        s = np.zeros(6)
        native.check(lib.phovo_odometry_get_optimal_state_vector(h, s.ctypes.data_as(C.POINTER(C.c_double))), "state")
        got.append(s)
        native.check(lib.phovo_odometry_get_semidense_report(h, C.byref(rep)), "report")
        sels.append(list(rep.selected[:nl]))
        ps, ss = native.PairSystem(), native.SampledSystem()
        assert lib.phovo_odometry_get_pair_system(h, C.byref(ps)) == native.E_UNSUPPORTED
        assert lib.phovo_odometry_get_sampled_system(h, C.byref(ss)) == native.E_UNSUPPORTED
        assert lib.phovo_odometry_get_objective_system(h, C.byref(ps)) == native.E_UNSUPPORTED
        assert lib.phovo_odometry_get_geometric_system(h, C.byref(native.GeometricSystem())) == native.E_UNSUPPORTED
        assert lib.phovo_odometry_get_inverse_system(h, C.byref(ps)) == native.E_UNSUPPORTED
        assert lib.phovo_odometry_get_robust_system(h, C.byref(native.RobustSystem())) == native.E_UNSUPPORTED
    finally:
        lib.phovo_odometry_destroy(h)
    with odometry.CPhotoconsistencyOdometrySemiDense(0) as po:
        po.SetConfiguration(ncfg)
        po.SetSemiDenseOptions(opt)
        assert list(po.GetSemiDenseOptions().min_pixel_gradient) == list(opt.min_pixel_gradient)
        po.SetIntrinsicMatrix(x["K"])
        po.SetSourceFrame(x["gray0"], x["depth0"])
        po.SetTargetFrame(x["gray1"], x["depth1"])
        po.Optimize()
        got.append(po.GetOptimalStateVector())
        sels.append(list(po.GetSemiDenseReport().selected[:nl]))
        with pytest.raises(native.PhovoError) as err:
            po.SetExtensions(native.make_extensions(huber_delta=[0.1] * nl))
        assert err.value.status == native.E_UNSUPPORTED
    poses = [_bits(v) for v in got]
    assert len(poses) == 4 and all(v == poses[0] for v in poses), poses
    assert poses[0] != _bits(np.zeros(6))
    assert all(v == sels[0] for v in sels) and min(sels[0]) > 0, sels


# ---- 9. a skipped level ----------------------------------------------------------------------------------------------
def test_a_skipped_level():
    p, _ = sc.carry_pair(False)
    nl, mi = 3, [5, 0, 5]
    with _engine(p["K"], 160, 120, 2, mi) as eng:
        _upload(eng, [p])
        tau = _taus(eng, 0, 0.25, nl)
        eng.set_semidense_options(native.make_semidense_options(tau))
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        ref = sc.precheck(pyr, p["K"], sc.cfg(mi), tau)
        s, reps, sel = _align(eng, [0])
        assert [l["levels"] for l in eng.last_launches()] == [[2], [0]]           # no launch names level 1
    assert ref["selected"][1] == 0 and int(sel[0][1]) == 0 and ref["selected"][0] > 0 and ref["selected"][2] > 0
    _hold(s[0], reps[0], sel[0], ref, nl)


# ---- 10. per-level thresholds ----------------------------------------------------------------------------------------
def test_thresholds_belong_to_their_levels():
    p = synthetic.make_pair(5, 80, 60, holes=0.02)
    nl, mi = 2, [6, 6]
    out = []
    with _engine(p["K"], 80, 60, 2, mi) as eng:
        _upload(eng, [p])
        ta, tb = _taus(eng, 0, 0.5, nl)[0], _taus(eng, 0, 0.05, nl)[0]
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        for tau in ([ta, tb], [tb, ta]):
            eng.set_semidense_options(native.make_semidense_options(tau))
            ref = sc.precheck(pyr, p["K"], sc.cfg(mi), tau)
            s, reps, sel = _align(eng, [0])
            _hold(s[0], reps[0], sel[0], ref, nl)
            out.append((s[0], ref))
    ratio = np.abs(out[0][0] - out[1][0]).max() / sr.pose_bar(out[0][1]["cond"], out[0][1]["state"])
    print(f"[tau_a, tau_b] against [tau_b, tau_a]: {ratio:.3g} bars; selected {out[0][1]['selected']} / {out[1][1]['selected']}")
    assert ratio > 1000.0 and out[0][1]["selected"] != out[1][1]["selected"]


# ---- 11. refusals ----------------------------------------------------------------------------------------------------
UNSUPPORTED_EXTENSIONS = [dict(plane_storage=native.STORAGE_F32), dict(plane_storage=native.STORAGE_F16),
                          dict(sampling=native.SAMPLING_BILINEAR),
                          dict(sampling=native.SAMPLING_BILINEAR, jacobian_corrected=True),
                          dict(huber_delta=[0.05] * 4)]


@pytest.mark.parametrize("ext", UNSUPPORTED_EXTENSIONS)
def test_unsupported_extensions_are_refused_in_both_orders(ext):
    x = native.make_extensions(**ext)
    with odometry.AlignmentEngine() as eng:
        eng.set_objective(SEMI)
        assert _status(eng.set_extensions, x) == native.E_UNSUPPORTED
        assert eng.get_objective() == SEMI
    with odometry.AlignmentEngine() as eng:
        eng.set_extensions(x)
        assert _status(eng.set_objective, SEMI) == native.E_UNSUPPORTED
        assert eng.get_objective() == native.OBJECTIVE_PHOTOMETRIC


def test_refusals_and_the_pool_survives_the_round_trip():
    p = synthetic.make_pair(9, 80, 60, holes=0.02)
    ncfg = native.make_config(num_levels=2, max_iter=[5, 5], min_grad=[0.0, 0.0])
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_intrinsic_matrix(p["K"])
        # bad options: refused under any objective, the ones in force stay
        for bad in (-1.0, float("nan"), float("inf")):
            opt = native.make_semidense_options()
            opt.min_pixel_gradient[1] = bad
            assert _status(eng.set_semidense_options, opt) == native.E_INVALID_ARGUMENT
        assert list(eng.get_semidense_options().min_pixel_gradient) == [0.0] * native.MAX_LEVELS
        assert _status(eng.fetch_semidense_reports, 1) == native.E_NOT_READY            # nothing enqueued yet
        eng.reserve_frames(2, 80, 60)
        eng.upload_frame(0, p["gray0"], p["depth0"])
        eng.upload_frame(1, p["gray1"], p["depth1"])
        before = eng.align_pairs([0], [1])                                      # objective 0
        assert _status(eng.fetch_semidense_reports, 1) == native.E_UNSUPPORTED
        eng.set_objective(SEMI)                                                 # 0 -> 7: the pool stays
        assert eng.level_is_stored(1)
        tau = odometry.semidense_thresholds(eng, 0, 0.25)
        eng.set_semidense_options(native.make_semidense_options(tau))
        semi = eng.align_pairs([0], [1])
        assert {l["kind"] for l in eng.last_launches()} == {"inverse_semidense"}
        assert _status(eng.fetch_semidense_reports, 2) == native.E_INVALID_ARGUMENT
        zero6, zero8 = np.zeros((1, 6)), np.zeros((1, 8))
        assert _status(eng.evaluate_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_sampled_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_sampled_pairs, [0], [1], zero8, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_objective_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_geometric_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_inverse_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_robust_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.enqueue_align, [0], [1], None, np.zeros((1, 6)), np.eye(6)[None]) == native.E_UNSUPPORTED
        # fusion, sliding-window, wide, latency-form and batch-invariant settings: accepted, no effect
        eng.set_level_fusion(native.FUSION_OFF); eng.set_wide_policy(1); eng.set_latency_forms(True)
        eng.set_batch_invariant(True); eng.set_slide_policy(-1)
        assert _bits(eng.align_pairs([0], [1])) == _bits(semi)
        eng.set_level_fusion(native.FUSION_AUTO); eng.set_wide_policy(0); eng.set_latency_forms(False)
        eng.set_batch_invariant(False); eng.set_slide_policy(0)
        eng.set_objective(INVERSE)                                              # 7 -> 5
        assert eng.level_is_stored(1)
        inverse = eng.align_pairs([0], [1])
        assert _status(eng.fetch_semidense_reports, 1) == native.E_UNSUPPORTED
        eng.set_objective(SEMI)                                                 # 5 -> 7: the options are still in force
        assert eng.level_is_stored(1)
        assert _bits(eng.align_pairs([0], [1])) == _bits(semi)
        eng.set_objective(native.OBJECTIVE_PHOTOMETRIC)                         # 7 -> 0
        assert eng.level_is_stored(1)
        after = eng.align_pairs([0], [1])
    assert _bits(before) == _bits(after)
    assert len({repr(_bits(v)) for v in (before, semi, inverse)}) == 3


def test_a_source_without_gradients_is_not_ready():
    p = synthetic.make_pair(9, 80, 60, holes=0.02)
    with _engine(p["K"], 80, 60, 2, [5, 5]) as eng:
        eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
        eng.upload_frame(1, p["gray1"], p["depth1"], roles=native.ROLE_TARGET)
        assert _status(eng.align_pairs, [0], [1]) == native.E_NOT_READY
        eng.upload_frame(0, p["gray0"], p["depth0"])                            # both roles
        s = eng.align_pairs([0], [1])
        assert np.all(np.isfinite(s)) and np.any(s != 0.0)


def test_thresholds_follow_the_engines_depth_range():
    """semidense_thresholds takes its quantile over the pixels the kernel's depth gate admits: under set_depth_range(0.5, 2.0)
    it is the quantile of that range (not of the default 0.3 ... 5.0), the device selects a quarter of THOSE pixels, and the
    result holds the checker under the same range."""
    p = synthetic.make_pair(5, 80, 60, holes=0.02)
    nl, mi, rng = 2, [6, 6], (0.5, 2.0)
    with _engine(p["K"], 80, 60, 2, mi, depth_range=rng) as eng:
        _upload(eng, [p])
        tau = _taus(eng, 0, 0.25, nl)
        assert tau == odometry.semidense_thresholds(eng, 0, 0.25, min_depth=rng[0], max_depth=rng[1])[:nl]
        assert tau != odometry.semidense_thresholds(eng, 0, 0.25, min_depth=0.3, max_depth=5.0)[:nl]
        eng.set_semidense_options(native.make_semidense_options(tau))
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        ref = sc.precheck(pyr, p["K"], sc.cfg(mi, None, *rng), tau)
        s, reps, sel = _align(eng, [0])
    _hold(s[0], reps[0], sel[0], ref, nl)
    for L in range(nl):
        d = pyr[L][1]
        valid = int(((d > rng[0]) & (d < rng[1])).sum())
        assert 0 < valid < d.size and abs(ref["selected"][L] / valid - 0.25) < 0.02, (L, valid, ref["selected"])
