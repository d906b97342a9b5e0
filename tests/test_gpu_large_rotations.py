"""Alignments at large rotations against the oracle (run with -m gpu on an MI355X).

The rest of the suite keeps Euler angles below 0.3 rad, i.e. inside the first of the three ways the device takes to sin /
cos (write_pose_constants, gn_device.hpp; tests/test_gpu_pose_constants.py holds the function itself to exact arithmetic).
Here whole alignments run with initial states and true motions in every branch -- polynomials below 0.3 and up to
fl(pi/4), the library's sincos beyond -- and with pitch / roll beyond pi/2, where points land behind the camera (Z < 0:
the reference has no Z > 0 gate, mirrored projections count).  Every case holds identical iteration counts and the
conditioned pose bar of tests/tools/fuzz_parity.py, 1e-9 x max(1, cond(J^T J) / 1e5); every case is checked to be
well-posed for that bar: one ulp of fx moves the oracle's own result by less than a quarter of it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_states
import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P4 = 0.78539816339744828


def _cfgs(max_iter, min_grad):
    nl = len(max_iter)
    return (native.make_config(num_levels=nl, max_iter=max_iter, min_grad=min_grad),
            oracle.make_config(num_levels=nl, max_iter=max_iter, min_grad=min_grad))


def _cond(trace):
    c = 1.0
    for e in trace:
        h = e["hessian"]
        if np.all(np.isfinite(h)) and np.any(h != 0.0):
            c = max(c, float(np.linalg.cond(h)))
    return c


class Expect:
    """The oracle's result for one case on the given pyramids (or stored planes), its bar, and its well-posedness."""

    def __init__(self, ocfg, K, planes, init, **ext):
        self.max_iter = [ocfg.max_num_iterations[l] for l in range(ocfg.num_levels)]
        self.state, self.its, tr = oracle.optimize(ocfg, K, *planes, init_state=init, want_trace=True, **ext)
        self.valid = oracle.valid_pixels_per_level(tr, ocfg.num_levels)
        self.finite = bool(np.all(np.isfinite(self.state)))
        self.bar = min(1e-5, 1e-9 * max(1.0, _cond(tr) / 1e5))
        if self.finite:
            K1 = K.copy()
            K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
            s1, _ = oracle.optimize(ocfg, K1, *planes, init_state=init, **ext)
            sens = se3.state_distance(self.state, s1) if np.all(np.isfinite(s1)) else np.inf
            assert sens < 0.25 * self.bar, f"chaotic case: one ulp of fx moves the oracle by {sens:.3e}, bar {self.bar:.1e}"

    def check(self, state, rep, what):
        nl = len(self.its)
        its = list(rep.iterations[:nl])
        assert list(rep.valid_pixels[:nl]) == self.valid, (what, list(rep.valid_pixels[:nl]), self.valid)
        if not self.finite:
            # No valid pixel (the scene behind or beside the camera): both sides end with a non-finite state, the device's
            # flagged.  The reference keeps iterating on the NaN, the device stops at the first one:
            # its counts are at most the oracle's.
            assert rep.flags & native.PAIR_NONFINITE and not np.all(np.isfinite(state)), (what, rep.flags, state)
            assert all(d <= o for d, o in zip(its, self.its)), (what, its, self.its)
            return
        assert its == self.its, (what, its, self.its)
        assert not rep.flags & native.PAIR_NONFINITE, (what, rep.flags)
        executed = [l for l in range(nl) if self.max_iter[l] > 0]
        deficient = any(self.valid[l] < 6 for l in executed)
        assert bool(rep.flags & native.PAIR_RANK_DEFICIENT) == deficient, (what, rep.flags, self.valid)
        d = se3.state_distance(state, self.state)
        assert d < self.bar, (what, d, self.bar)


def _upload(eng, p, w, h):
    eng.set_intrinsic_matrix(p["K"])
    eng.reserve_frames(2, w, h)
    eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
    eng.upload_frame(1, p["gray1"], None, roles=native.ROLE_TARGET)


def _pyramids(ocfg, p):
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    return i0p, d0p, i1p, gxp, gyp


def _stored_planes(eng, mi, w, h):
    """Oracle inputs = exactly the planes the device holds (rounded to the storage type); levels it does not hold: zeros."""
    planes = [[], [], [], [], []]
    for l in range(len(mi)):
        if mi[l] > 0:
            i0, d0, _, _ = eng.get_level_planes(0, l)
            i1, _, gx, gy = eng.get_level_planes(1, l)
        else:
            lw, lh = oracle.level_size(w, h, l)
            i0 = d0 = i1 = gx = gy = np.zeros((lh, lw))
        for lst, v in zip(planes, (i0, d0, i1, gx, gy)):
            lst.append(v)
    return planes


_initial_states = edge_states.initial_states


# ------------------------------------------------------------------------------------------------------------------------
# initial states in every branch, fixed iterations
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,latency_kind", [((80, 60), "persistent"), ((160, 120), "wide")])
def test_initial_states_in_every_branch(size, latency_kind):
    """32 initial states (branches 2 and 3 on each axis, both signs, and two behind the camera), three fixed iterations on a
    level whose owner map sits in LDS: nine pairs per launch (the throughput geometry) and one pair in the latency forms
    (at 160x120 that is the wide form)."""
    w, h = size
    p = synthetic.make_pair(61, w, h, holes=0.02, trans=0.01, rot=0.004)
    ncfg, ocfg = _cfgs([3], [0.0])
    inits = _initial_states()
    planes = _pyramids(ocfg, p)
    expect = [Expect(ocfg, p["K"], planes, s) for s in inits]
    assert any(not e.finite or e.valid[0] < w * h // 4 for e in expect)          # some states see (almost) nothing
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        _upload(eng, p, w, h)
        assert eng.level_launch_info(0)["owner_in_lds"]
        for g in range(0, len(inits), 9):
            idx = [(g + k) % len(inits) for k in range(9)]
            s, reps = eng.align_pairs([0] * 9, [1] * 9, init_states=np.stack([inits[i] for i in idx]), want_reports=True)
            assert [r["kind"] for r in eng.last_launches()] == ["persistent"]
            for k, i in enumerate(idx):
                expect[i].check(s[k], reps[k], ("nine", size, i, inits[i][3:]))
        eng.set_latency_forms(True)
        for i, st in enumerate(inits):
            s, reps = eng.align_pairs([0], [1], init_states=st[None], want_reports=True)
            assert [r["kind"] for r in eng.last_launches()] == [latency_kind]
            expect[i].check(s[0], reps[0], ("one", size, i, st[3:]))


def test_initial_states_in_every_branch_through_the_fused_launch():
    """Two levels (160x120, 80x60) in one fused launch, nine pairs, a threshold that does not end them early."""
    w, h = 320, 240
    p = synthetic.make_pair(62, w, h, holes=0.02, trans=0.01, rot=0.004)
    ncfg, ocfg = _cfgs([0, 3, 3], [1e-9, 1e-9, 1e-9])
    inits = _initial_states()
    planes = _pyramids(ocfg, p)
    expect = [Expect(ocfg, p["K"], planes, s) for s in inits]
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        _upload(eng, p, w, h)
        for g in range(0, len(inits), 9):
            idx = [(g + k) % len(inits) for k in range(9)]
            s, reps = eng.align_pairs([0] * 9, [1] * 9, init_states=np.stack([inits[i] for i in idx]), want_reports=True)
            assert [r["kind"] for r in eng.last_launches()] == ["fused"]
            for k, i in enumerate(idx):
                expect[i].check(s[k], reps[k], ("fused", i, inits[i][3:]))


# ------------------------------------------------------------------------------------------------------------------------
# true in-plane motions of 0.5, 0.7, 0.9 rad, converging
# ------------------------------------------------------------------------------------------------------------------------
MOTIONS, NEAR = edge_states.MOTIONS, edge_states.NEAR                              # yaw 0.5, 0.7, 0.9: branches 2, 2, 3


@pytest.mark.parametrize("bilinear,huber", [(False, None), (True, None), (True, [0.05])])
@pytest.mark.parametrize("storage", [native.STORAGE_F64, native.STORAGE_F32, native.STORAGE_F16])
def test_large_in_plane_motions_on_every_storage(storage, bilinear, huber):
    """Rendered pairs under an in-plane rotation of 0.5, 0.7 and 0.9 rad, started near the truth, ended by the gradient
    threshold: nearest-neighbour and bilinear sampling (with and without Huber weights) on fp64 / fp32 / fp16 planes."""
    w, h = 160, 120
    mi, mg = [30], [2.0]
    ncfg, ocfg = _cfgs(mi, mg)
    ext = dict(huber_delta=huber, bilinear=bilinear)
    by_threshold = 0
    for j, m in enumerate(MOTIONS):
        p = synthetic.render_pair_with_motion(70 + j, w, h, m)
        init = p["motion"] + NEAR
        with odometry.AlignmentEngine() as eng:
            eng.set_config(ncfg)
            eng.set_extensions(native.make_extensions(
                plane_storage=storage, huber_delta=huber,
                sampling=native.SAMPLING_BILINEAR if bilinear else native.SAMPLING_NEAREST_SCATTER))
            _upload(eng, p, w, h)
            planes = _stored_planes(eng, mi, w, h)
            s, reps = eng.align_pairs([0] * 9, [1] * 9, init_states=np.tile(init, (9, 1)), want_reports=True)
            assert [r["kind"] for r in eng.last_launches()] == ["bilinear" if bilinear else "persistent"]
        e = Expect(ocfg, p["K"], planes, init, **ext)
        assert e.finite and abs(e.state[3] - m[3]) < 0.05
        by_threshold += e.its[0] < mi[0]
        for k in range(9):
            e.check(s[k], reps[k], (m[3], k))
            assert np.array_equal(s[k], s[0])
    assert by_threshold >= 2                    # (nearest-neighbour sampling at 0.9 rad may circle the truth to the cap)


def test_large_in_plane_motions_through_the_wide_form():
    """One pair at 640x480 (the wide form: several workgroups on one level), in-plane rotations of 0.5 / 0.7 / 0.9 rad."""
    w, h = 640, 480
    mi, mg = [30], [20.0]
    ncfg, ocfg = _cfgs(mi, mg)
    by_threshold = 0
    for j, m in enumerate(MOTIONS):
        p = synthetic.render_pair_with_motion(75 + j, w, h, m)
        init = p["motion"] + NEAR
        e = Expect(ocfg, p["K"], _pyramids(ocfg, p), init)
        with odometry.AlignmentEngine() as eng:
            eng.set_config(ncfg)
            _upload(eng, p, w, h)
            s, reps = eng.align_pairs([0], [1], init_states=init[None], want_reports=True)
            assert [r["kind"] for r in eng.last_launches()] == ["wide"]
        assert e.finite and abs(e.state[3] - m[3]) < 0.05
        by_threshold += e.its[0] < mi[0]
        e.check(s[0], reps[0], ("wide", m[3]))
    assert by_threshold >= 1


# ------------------------------------------------------------------------------------------------------------------------
# the sliding-window kernel at 320x240
# ------------------------------------------------------------------------------------------------------------------------
def test_sliding_window_hands_rolls_of_either_sign_and_pi_over_4_crossings_to_the_exact_kernel():
    """A roll shifts whole rows and the window is asymmetric (about 24 rows behind the source's band, 6 ahead at 320x240):
    a roll of +0.12 and one of -0.12 leave it through different sides.  A pair started at yaw 0.70 towards a true 0.9
    crosses fl(pi/4) within the launch, but in the EXACT kernel: an in-plane rotation of 0.7 rad moves the border pixels by
    some 100 rows, so it leaves the window in its first iteration and the exact kernel does all of its iterations (pinned:
    its bits are those of a launch with the sliding-window kernel switched off).  No pair of this size can cross pi/4 in yaw
    and stay inside a window of 30 rows.  All must be finished by the exact kernel with the oracle's result; a well-behaved
    pair in the same launch is not touched: flags 0, the bits of a launch without the others."""
    w, h = 320, 240
    roll_p = synthetic.render_pair_with_motion(81, w, h, [0.005, 0.004, -0.003, 0.004, 0.003, 0.12])
    roll_m = synthetic.render_pair_with_motion(82, w, h, [0.005, 0.004, -0.003, 0.004, 0.003, -0.12])
    cross = synthetic.render_pair_with_motion(83, w, h, [0.01, -0.005, 0.004, 0.9, 0.002, -0.003])
    small = synthetic.make_pair(84, w, h, holes=0.02, trans=0.01, rot=0.004)
    probs = [roll_p, roll_m, cross, small]
    inits = [roll_p["motion"] + NEAR, roll_m["motion"] + NEAR, np.array([0.0, 0.0, 0.0, 0.70, 0.0, 0.0]), np.zeros(6)]
    ncfg, ocfg = _cfgs([8], [0.0])
    expect = [Expect(ocfg, p["K"], _pyramids(ocfg, p), i) for p, i in zip(probs, inits)]
    assert expect[2].state[3] > P4                                         # the crossing case did cross
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_intrinsic_matrix(small["K"])
        eng.reserve_frames(8, w, h)
        for i, p in enumerate(probs):
            eng.upload_frame(2 * i, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
            eng.upload_frame(2 * i + 1, p["gray1"], None, roles=native.ROLE_TARGET)
        assert not eng.level_launch_info(0)["owner_in_lds"]
        which = [k % 4 for k in range(48)]
        s, reps = eng.align_pairs([2 * c for c in which], [2 * c + 1 for c in which],
                                  init_states=np.stack([inits[c] for c in which]), want_reports=True)
        assert [r["kind"] for r in eng.last_launches()] == ["slide", "slide_fallback"]
        alone = eng.align_pairs([6] * 48, [7] * 48)
        eng.set_slide_policy(-1)
        exact = eng.align_pairs([2 * c for c in which], [2 * c + 1 for c in which],
                                init_states=np.stack([inits[c] for c in which]))
        assert "slide" not in [r["kind"] for r in eng.last_launches()]
    for k, c in enumerate(which):
        expect[c].check(s[k], reps[k], ("slide", k, c))
        if c < 3:
            assert reps[k].flags == native.PAIR_WINDOW_FALLBACK, (k, c, reps[k].flags)
        else:
            assert reps[k].flags == 0 and np.array_equal(s[k], alone[0]), (k, reps[k].flags)
        if c == 2:                                   # the crossing pair: all its iterations ran in the exact kernel
            assert np.array_equal(s[k], exact[k]), (k, s[k], exact[k])


# ------------------------------------------------------------------------------------------------------------------------
# non-finite initial angles in one pair of a launch, every kernel form
# ------------------------------------------------------------------------------------------------------------------------
# (form, size, max_iter, min_grad, storage, bilinear, wide policy, pairs, launch kinds).  Pass 1 of every form keeps a NaN or
# saturated coordinate away from any address ("Non-finite states"): the bad pair sees no valid pixel.
NONFINITE_FORMS = [
    ("persistent", (80, 60), [3], [0.0], native.STORAGE_F64, False, 0, 9, ["persistent"]),
    ("fused", (320, 240), [0, 3, 3], [1e-9] * 3, native.STORAGE_F64, False, 0, 9, ["fused"]),
    ("slide", (320, 240), [3], [0.0], native.STORAGE_F64, False, 0, 40, ["slide"]),
    ("wide", (160, 120), [3], [0.0], native.STORAGE_F64, False, 1, 9, ["wide"]),
    ("bilinear_dma_f64", (80, 60), [3], [0.0], native.STORAGE_F64, True, 0, 9, ["bilinear"]),
    ("bilinear_dma_f32", (80, 60), [3], [0.0], native.STORAGE_F32, True, 0, 9, ["bilinear"]),
    ("bilinear_records_f16", (80, 60), [3], [0.0], native.STORAGE_F16, True, 0, 9, ["bilinear"]),
]


@pytest.mark.parametrize("form,size,mi,mg,storage,bilinear,wide,pairs,kinds", NONFINITE_FORMS, ids=[f[0] for f in NONFINITE_FORMS])
def test_non_finite_initial_angle_in_one_pair_of_a_launch(form, size, mi, mg, storage, bilinear, wide, pairs, kinds):
    """NaN yaw, +inf pitch, -inf roll as the initial state of one pair (phovo_engine_align_pairs passes init_states to the
    device unchecked): that pair ends non-finite and flagged PHOVO_PAIR_NONFINITE with the oracle's valid-pixel counts (0:
    every coordinate is NaN) and at most its iteration counts (the device stops at the first non-finite state, the
    reference keeps iterating on it); every other pair of the launch is bit for bit what it is when the bad pair's state
    is finite, and matches the oracle."""
    w, h = size
    p = synthetic.make_pair(64, w, h, holes=0.02, trans=0.01, rot=0.004)
    ncfg, ocfg = _cfgs(mi, mg)
    good = np.array([0.01, -0.02, 0.015, 0.02, -0.01, 0.015])
    bad_at = 4
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_extensions(native.make_extensions(
            plane_storage=storage, sampling=native.SAMPLING_BILINEAR if bilinear else native.SAMPLING_NEAREST_SCATTER))
        if wide:
            eng.set_wide_policy(wide)
        _upload(eng, p, w, h)
        planes = _stored_planes(eng, mi, w, h)
        inits = np.tile(good, (pairs, 1))
        clean = eng.align_pairs([0] * pairs, [1] * pairs, init_states=inits)
        results = []
        for axis, bad in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            st = inits.copy()
            st[bad_at, 3 + axis] = bad
            s, reps = eng.align_pairs([0] * pairs, [1] * pairs, init_states=st, want_reports=True)
            assert [r["kind"] for r in eng.last_launches()][:len(kinds)] == kinds, (form, eng.last_launches())
            results.append((st[bad_at], s, reps))
    ext = dict(bilinear=True) if bilinear else {}
    e_good = Expect(ocfg, p["K"], planes, good, **ext)
    for st, s, reps in results:
        e_bad = Expect(ocfg, p["K"], planes, st, **ext)
        assert not e_bad.finite and all(v == 0 for v in e_bad.valid)
        e_bad.check(s[bad_at], reps[bad_at], (form, "bad", st[3:]))
        for k in range(pairs):
            if k != bad_at:
                assert np.array_equal(s[k], clean[k]), (form, k, st[3:])
                assert reps[k].flags & native.PAIR_NONFINITE == 0
        e_good.check(s[0], reps[0], (form, "good", st[3:]))


# ------------------------------------------------------------------------------------------------------------------------
# the class surface
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angles", [(0.55, 0.0, 0.0), (0.0, 0.783, -0.80), (-1.2, 0.31, 0.0), (0.0, 0.0, np.pi - 0.3)])
def test_class_surface_pose_matrix_at_large_states(angles):
    """Optimize() through the class-shaped surface from a large initial state: the state matches the oracle and
    GetOptimalRigidTransformationMatrix is the oracle's eigen_pose of it to 1e-15."""
    w, h = 80, 60
    p = synthetic.make_pair(63, w, h, holes=0.02, trans=0.01, rot=0.004)
    ncfg, ocfg = _cfgs([3], [0.0])
    init = np.array([0.01, -0.02, 0.015, *angles])
    e = Expect(ocfg, p["K"], _pyramids(ocfg, p), init)
    with odometry.CPhotoconsistencyOdometryAnalytic() as po:
        po.SetConfiguration(ncfg)
        po.SetIntrinsicMatrix(p["K"])
        po.SetSourceFrame(p["gray0"], p["depth0"])
        po.SetTargetFrame(p["gray1"], p["depth1"])
        po.SetInitialStateVector(init)
        po.Optimize()
        state = po.GetOptimalStateVector()
        rep = po.GetReport()
        rt = po.GetOptimalRigidTransformationMatrix()
    e.check(state, rep, ("class", angles))
    if e.finite:
        np.testing.assert_allclose(rt, oracle.eigen_pose(state), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------------
# fuzzing across the branches
# ------------------------------------------------------------------------------------------------------------------------
def test_randomised_sweep_of_large_angles_against_oracle():
    """tests/tools/fuzz_parity.py in its `angles` mode: 60 problems with initial Euler angles drawn in every branch of the
    device's sin / cos, near both thresholds and behind the camera, and true in-plane motions up to 0.9 rad."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "fuzz_parity.py"), "60", "17", "angles"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "60 cases, 0 failures" in r.stdout
    print(r.stdout.strip().splitlines()[-5])
