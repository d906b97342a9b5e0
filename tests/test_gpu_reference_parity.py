"""The HIP path against the reference build, directly (run with -m gpu on an MI355X).

oracle/_ref/libphovo_ref.so is the reference's own Analytic and BiObjective headers compiled unmodified over stand-in
headers (oracle/Makefile.ref).  It travels with the working tree; the reference tree itself is never read here, and neither
is the oracle: every expectation below comes out of that library through its C surface (oracle/reference_build.py).

Held: analytic and bi-objective alignments to pose distance <= 1e-9 with equal iteration counts per level, in the fused,
level (persistent), slide and wide kernel forms; phovo_eigen_pose and the device's pose constants to the bars of
tests/test_gpu_pose_constants.py; the warp kernels (scatter + gather) bit for bit at levels 0-3; a seeded sweep of the
draws tests/test_reference_build_cpu.py uses.  Where the reference build ends non-finite (no valid pixel), the device must
flag it and end non-finite too; it stops at the first NaN, so its counts are at most the reference's.
Every test prints the largest distance it met.  The non-finite cases are also held to the same non-finite components.
"""
import ctypes as C
import glob
import os
import sys

import mpmath
import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import reference_build as refb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import fuzz_draws  # noqa: E402
import test_gpu_pose_constants as pc  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not refb.available(),
                                 reason="REFERENCE BUILD ABSENT: oracle/_ref/libphovo_ref.so did not travel with the tree; "
                                        "nothing here compared the HIP path with the reference")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "config_files")
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "case_*.npz")))
POSE_TOL = 1e-9


def _cfgs(**kw):
    """The device's configuration and the reference build's; the depth gate travels in the latter (set_depth_range)."""
    return native.make_config(**{k: v for k, v in kw.items() if k not in ("min_depth", "max_depth")}), refb.make_config(**kw)


def _yml(name, max_iter=None, min_grad=None):
    n = native.read_config_file(os.path.join(CFG_DIR, name))
    nl = n.num_levels
    return _cfgs(num_levels=nl, blur=list(n.blur_filter_size[:nl]), grad_scale=list(n.image_gradients_scaling_factor[:nl]),
                 lam=list(n.lambda_optimization_step[:nl]),
                 max_iter=list(n.max_num_iterations[:nl]) if max_iter is None else max_iter,
                 min_grad=list(n.min_gradient_norm[:nl]) if min_grad is None else min_grad)


def _check(what, kind, state, rep, es, eits):
    nl = len(eits)
    its = list(rep.iterations[:nl])
    if not np.all(np.isfinite(es)):
        assert rep.flags & native.PAIR_NONFINITE, (what, rep.flags, state, es)
        assert np.array_equal(np.isfinite(state), np.isfinite(es)), (what, state, es)      # the same components
        assert all(d <= r for d, r in zip(its, eits)), (what, its, eits)
        return 0.0
    assert its == eits, (what, its, eits)
    d = se3.state_distance(state, es)
    assert d <= POSE_TOL, (what, d)
    return d


def _align_on_device(ncfg, K, g0, d0, g1, d1, inits, n_pairs, biobjective=False, latency=False, depth_range=None):
    """One engine, one pair of frames, n_pairs copies of the pair (with the given initial states, cycled)."""
    h, w = g0.shape
    with odometry.AlignmentEngine(0) as eng:
        eng.set_config(ncfg)
        eng.set_intrinsic_matrix(K)
        if depth_range is not None:
            eng.set_depth_range(*depth_range)
        if biobjective:
            eng.set_objective(native.OBJECTIVE_BIOBJECTIVE)
        if latency:
            eng.set_latency_forms(True)
        eng.reserve_frames(2, w, h)
        eng.upload_frame(0, g0, d0, roles=native.ROLE_SOURCE)
        eng.upload_frame(1, g1, d1 if biobjective else None, roles=native.ROLE_TARGET)
        init = None if inits is None else np.stack([inits[k % len(inits)] for k in range(n_pairs)])
        states, reps = eng.align_pairs([0] * n_pairs, [1] * n_pairs, init_states=init, want_reports=True)
        kinds = [r["kind"] for r in eng.last_launches()]
    return states, reps, kinds


def _parity(what, ncfg, rcfg, K, g0, d0, g1, d1=None, inits=None, n_pairs=1, biobjective=False, latency=False):
    ref_align = refb.biobjective_align if biobjective else refb.analytic_align
    kind = "biobjective" if biobjective else "analytic"
    starts = [None] if inits is None else list(inits)
    expect = [ref_align(rcfg, K, g0, d0, g1, d1, s)[:2] for s in starts]
    states, reps, kinds = _align_on_device(ncfg, K, g0, d0, g1, d1, inits, n_pairs, biobjective, latency,
                                           (rcfg.min_depth, rcfg.max_depth))
    worst = 0.0
    for k in range(n_pairs):
        es, eits = expect[k % len(expect)]
        worst = max(worst, _check((what, k), kind, states[k], reps[k], es, eits))
    print(f"{what}: {n_pairs} pairs, launches {kinds}, worst distance to the reference build {worst:.3e}")
    return kinds


# ------------------------------------------------------------------------------------------------------------------------
# analytic aligner
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_cases(path):
    d = np.load(path)
    nl = int(d["num_levels"])
    ncfg, rcfg = _cfgs(num_levels=nl, blur=[0] * nl, grad_scale=list(d["grad_scale"]), lam=list(d["lam"]),
                       max_iter=[int(v) for v in d["max_iter"]], min_grad=list(d["min_grad"]),
                       min_depth=float(d["min_depth"]), max_depth=float(d["max_depth"]))
    for n_pairs in (1, 9):
        _parity(os.path.basename(path), ncfg, rcfg, d["K"], d["gray0"], d["depth0"], d["gray1"], inits=[d["init_state"]],
                n_pairs=n_pairs)


@pytest.mark.parametrize("n_pairs", [1, 32, 33], ids=lambda n: f"{n} pairs")
@pytest.mark.parametrize("max_iter,min_grad", [(None, None), ([0, 0, 20, 50], [0.0] * 4)], ids=["shipped", "fixed 50+20"])
def test_640x480_four_levels(max_iter, min_grad, n_pairs):
    """Levels 2 and 3 (160x120, 80x60): the fused launch with the shipped thresholds, one level kernel per level otherwise."""
    ncfg, rcfg = _yml("config_4_level_optimization_analytic.yml", max_iter, min_grad)
    p = synthetic.make_pair(1, 640, 480, holes=0.05)
    _parity(("640x480", n_pairs), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], n_pairs=n_pairs)


@pytest.mark.parametrize("n_pairs", [1, 32, 33], ids=lambda n: f"{n} pairs")
def test_both_sides_of_the_wide_rule(n_pairs):
    """320x240 at level 0 is beyond what one workgroup's LDS holds: n_pairs <= 32 selects the wide form (several workgroups
    per pair), 33 the sliding window."""
    p = synthetic.make_pair(350, 320, 240, holes=0.02)
    ncfg, rcfg = _cfgs(num_levels=3, max_iter=[3, 5, 8], min_grad=[0.0] * 3)
    kinds = _parity(("320x240", n_pairs), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], n_pairs=n_pairs)
    assert ("wide" in kinds) == (n_pairs <= 32), kinds
    assert ("slide" in kinds) == (n_pairs > 32), kinds


def test_640x480_level_zero_in_the_slide_form():
    ncfg, rcfg = _yml("config_only_level_0_analytic.yml")
    p = synthetic.make_pair(2, 640, 480)
    kinds = _parity("640x480 level 0", ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], n_pairs=40)
    assert "slide" in kinds, kinds


@pytest.mark.parametrize("size", [(320, 240), (160, 120), (200, 152), (75, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smaller_shapes(size):
    w, h = size
    p = synthetic.make_pair(30 + w, w, h, holes=0.02)
    for max_iter, min_grad in (([3, 5, 8], [0.0] * 3), ([10, 10, 10], [1.0, 30.0, 30.0])):
        ncfg, rcfg = _cfgs(num_levels=3, max_iter=max_iter, min_grad=min_grad)
        for n_pairs, latency in ((1, True), (9, False), (40, False)):
            _parity((size, max_iter, n_pairs), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], n_pairs=n_pairs,
                    latency=latency)


ROTATIONS = (0.31, 0.5, 0.78, 0.79, 1.2, 2.5)


def _rotated_states():
    out = []
    for axis in range(3):
        for k, a in enumerate(ROTATIONS):
            s = np.array([0.01, -0.02, 0.015, 0.002, -0.001, 0.003])
            s[3 + axis] = a if (k + axis) % 2 == 0 else -a
            out.append(s)
    return out


@pytest.mark.parametrize("size,latency", [((80, 60), False), ((160, 120), True), ((640, 480), False)],
                         ids=["80x60 nine per launch", "160x120 latency forms", "640x480 wide"])
def test_large_initial_rotations_on_each_axis(size, latency):
    w, h = size
    p = synthetic.make_pair(61, w, h, holes=0.02, trans=0.01, rot=0.004)
    inits = _rotated_states()
    if (w, h) == (640, 480):
        ncfg, rcfg = _cfgs(num_levels=4, max_iter=[0, 0, 3, 3], min_grad=[0.0] * 4)
        _parity(("rotations", size), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], inits=inits, n_pairs=len(inits))
        return
    ncfg, rcfg = _cfgs(num_levels=2, max_iter=[3, 3], min_grad=[0.0, 0.0])
    if latency:
        for i, s in enumerate(inits):
            _parity(("rotation", size, i), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], inits=[s], n_pairs=1,
                    latency=True)
    else:
        _parity(("rotations", size), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], inits=inits, n_pairs=len(inits))


# ------------------------------------------------------------------------------------------------------------------------
# bi-objective aligner
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter,min_grad", [(None, None), ([0, 0, 20, 50], [0.0] * 4)], ids=["shipped", "fixed 50+20"])
def test_biobjective_640x480(max_iter, min_grad):
    ncfg, rcfg = _yml("config_4_level_optimization_analytic.yml", max_iter, min_grad)
    for seed in (0, 1):
        p = synthetic.make_pair(seed, 640, 480, holes=0.05 if seed else 0.0)
        kinds = _parity(("bi 640x480", seed), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], p["depth1"], n_pairs=3,
                        biobjective=True)
        assert set(kinds) == {"biobjective"}


@pytest.mark.parametrize("size", [(320, 240), (160, 120), (200, 152), (75, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_biobjective_smaller_shapes(size):
    w, h = size
    p = synthetic.make_pair(30 + w, w, h, holes=0.02)
    for max_iter, min_grad in (([3, 5, 8], [0.0] * 3), ([10, 10, 10], [1.0, 30.0, 30.0])):
        ncfg, rcfg = _cfgs(num_levels=3, max_iter=max_iter, min_grad=min_grad)
        _parity(("bi", size, max_iter), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], p["depth1"], n_pairs=3,
                biobjective=True)


# ------------------------------------------------------------------------------------------------------------------------
# eigenPose and the device's pose constants
# ------------------------------------------------------------------------------------------------------------------------
# Rt(i, j) of the reference's eigenPose -> the device constant holding the same formula (sign)
RT_CONSTANTS = {(0, 1): ("R01", 1), (0, 2): ("R02", 1), (1, 1): ("R11", 1), (1, 2): ("R12", 1), (2, 1): ("T1", 1),
                (2, 2): ("T2", 1), (0, 0): ("T15", 1), (1, 0): ("T14", 1)}


def _bars(state, b):
    sc = {}
    for k, a in zip("ypr", state):
        sc["s" + k], sc["c" + k] = pc.exact_sincos(a)
    return {name: pc.composite_exact_and_bar(name, sc, 0.0, b)[1] for name in pc.COMPOSITES if name != "T11"}


def test_phovo_eigen_pose_against_the_reference_build():
    """Both sides evaluate the reference's formulas on the host's sin / cos (at most 1 ulp each): every entry within the
    sum of the two composite bars of tests/test_gpu_pose_constants.py at b = 1; translations and the last row exact."""
    rs = np.random.RandomState(4)
    states = [rs.uniform(-1, 1, 6) * s for s in (1e-3, 0.3, 1.0, 3.2) for _ in range(50)]
    states += [np.array([0.01, -0.02, 0.015, 0, 0, 0]) + np.eye(6)[3 + ax] * a for ax in range(3) for a in ROTATIONS]
    dp = C.POINTER(C.c_double)
    worst = 0.0
    for s in states:
        rt = np.zeros(16)
        assert native.lib().phovo_eigen_pose(np.ascontiguousarray(s).ctypes.data_as(dp), rt.ctypes.data_as(dp)) == 0
        rt, ref = rt.reshape(4, 4), refb.eigen_pose(s)
        assert np.array_equal(rt[:, 3], ref[:, 3]) and np.array_equal(rt[3], ref[3])
        bars = _bars(tuple(s[3:]), 1.0)
        for (i, j), (name, _) in RT_CONSTANTS.items():
            err = abs(mpmath.mpf(rt[i, j]) - mpmath.mpf(ref[i, j]))
            worst = max(worst, float(err / (2 * bars[name])))
            assert err <= 2 * bars[name], (s, name, rt[i, j], ref[i, j])
        assert abs(rt[2, 0] - ref[2, 0]) <= 2 * float(pc.ulp_of(mpmath.mpf(ref[2, 0])))
    print(f"phovo_eigen_pose: worst error / bar {worst:.3f}")


def test_device_pose_constants_against_the_reference_build(probe):
    """The constants write_pose_constants leaves on the device (tests/native/pose_constants_probe.hip) against the entries of
    the reference build's eigenPose that state the same formulas: within the device's bar (1 ulp per sin / cos on the
    polynomial branches, 2 on the library branch) plus the host's (1 ulp)."""
    mags = pc.small_magnitudes()[::8] + pc.SMALL_SPECIAL + pc.LARGE + list(ROTATIONS)
    states = pc.states_for(mags) + pc.mixed_states()[::3]
    rows = probe(states)
    worst = 0.0
    for state, row in zip(states, rows):
        sb = pc.branch_of_state(*state)
        b = max(pc.ULP_BAR[pc.branch_of_angle(a, sb)] for a in state)
        dev_bars, host_bars = _bars(state, b), _bars(state, 1.0)
        ref = refb.eigen_pose(pc.XYZ + tuple(state))
        assert tuple(row[:3]) == tuple(ref[:3, 3])
        for (i, j), (name, _) in RT_CONSTANTS.items():
            bar = dev_bars[name] + host_bars[name]
            err = abs(mpmath.mpf(row[pc.IDX[name]]) - mpmath.mpf(ref[i, j]))
            worst = max(worst, float(err / bar))
            assert err <= bar, (state, name, row[pc.IDX[name]], ref[i, j])
        exact_sp = pc.exact_sincos(state[1])[0]                       # Rt(2,0) = -sin(pitch), the device's T3 = sin(pitch)
        assert abs(mpmath.mpf(row[pc.IDX["T3"]]) + mpmath.mpf(ref[2, 0])) <= (b + 1.0) * pc.ulp_of(exact_sp), (state, "T3")
    print(f"device pose constants: {len(states)} states, worst error / bar {worst:.3f}")


probe = pc.probe


# ------------------------------------------------------------------------------------------------------------------------
# warp kernels
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", [(0, 0, 0, 0, 0, 0), (0.02, -0.01, 0.015, 0.01, -0.008, 0.006),
                                   (0.3, 0.2, 0.8, 0.2, -0.15, 0.4), (-0.1, 0.05, -1.2, 0.0, 0.0, 3.0)])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_warp_kernels_are_bit_exact(state, level):
    """phovo_warp_image runs the scatter kernel (owner map, last raster writer) and the gather kernel (owner -> intensity)."""
    p = synthetic.make_pair(11, 640, 480, holes=0.03)
    d = p["depth0"].copy()
    d[5, 7] = -1.0
    d[9, 9] = np.nan
    d[10, 10] = 1e-300
    rt = refb.eigen_pose(np.array(state, dtype=np.float64))
    got = odometry.warpImage(p["gray0"], d, rt, p["K"], level=level)
    exp = refb.warp_image(p["gray0"], d, rt, p["K"], level=level)
    assert got.dtype == np.uint8 and np.array_equal(got, exp)
    if level == 0:
        assert exp.any()


# ------------------------------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------------------------------
def test_sweep():
    """The draws of tests/test_reference_build_cpu.py (tests/tools/fuzz_draws.py), one, three or forty pairs per draw."""
    worst, nonfinite = 0.0, 0
    for index in range(200):
        case = fuzz_draws.reference_sweep_case(index)
        K, g0, d0, g1, d1 = fuzz_draws.reference_sweep_inputs(case, synthetic.make_pair)
        ncfg, rcfg = _cfgs(num_levels=case["num_levels"], max_iter=case["max_iter"], min_grad=case["min_grad"], lam=case["lam"])
        es, eits, _ = refb.analytic_align(rcfg, K, g0, d0, g1, None, case["init"])
        n_pairs = (1, 3, 40)[index % 3]
        states, reps, _ = _align_on_device(ncfg, K, g0, d0, g1, None, None if case["init"] is None else [case["init"]],
                                           n_pairs, latency=(index % 6 == 0))
        nonfinite += not np.all(np.isfinite(es))
        for k in range(n_pairs):
            worst = max(worst, _check(("sweep", index, k), "analytic", states[k], reps[k], es, eits))
    print(f"sweep: 200 draws ({nonfinite} non-finite in the reference build), worst distance {worst:.3e}")


def test_every_kernel_form_is_compared():
    """Self-contained: the shapes and batch sizes that select each analytic form, run here and held to the reference build."""
    seen = set()
    p = synthetic.make_pair(350, 320, 240, holes=0.02)
    ncfg, rcfg = _cfgs(num_levels=3, max_iter=[3, 5, 8], min_grad=[0.0] * 3)
    for n_pairs in (9, 40):                     # level kernels + wide; level kernels + sliding window and its hand-over
        seen.update(_parity(("forms 320x240", n_pairs), ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], n_pairs=n_pairs))
    ncfg, rcfg = _yml("config_4_level_optimization_analytic.yml")
    p = synthetic.make_pair(1, 640, 480, holes=0.05)
    seen.update(_parity("forms 640x480", ncfg, rcfg, p["K"], p["gray0"], p["depth0"], p["gray1"], n_pairs=9))
    assert {"fused", "persistent", "slide", "slide_fallback", "wide"} <= seen, seen
