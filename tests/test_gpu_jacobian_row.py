"""The analytic Jacobian row (analytic_row, csrc/gn_device.hpp) at large rotations and translations, in every kernel that
carries it (run with -m gpu on an MI355X).

The row's three rotation columns come from one cross product per pixel, Pr x Jt, contracted with three axes that depend
on the state only (yaw: e_z, pitch: (-sin yaw, cos yaw, 0), roll: Rt's first column).  What can go wrong is a sign or an
axis of that contraction, a constant read from the wrong slot, the bug term px * x of the reference's temp11 entering where
the reference's own temp15 terms have none, and one of the four kernel files forming the row differently from the others.
None of that shows at the small angles of the rest of the suite (at zero angles the three axes are e_z, e_y, e_x), so:

* the row itself: phovo_engine_evaluate_pairs returns J^T J, J^T r and the cost at given states.  One 160x120 pair with
  fy != fx on three levels, at a grid of states -- yaw, pitch or roll alone at +-0.3, +-0.8, +-1.5, +-2.8, mixed triples,
  each with translations of 0 and +-0.3 on x (the bug term), y and z -- against the oracle's residuals and Jacobians at
  the same state, at the bars of tests/test_gpu_pair_system.py.  Only states at which the oracle fills at least a quarter
  of the rows of EVERY level are in the grid (KEPT below was filtered with the oracle on the CPU; the test asserts the
  quarter again and skips nothing);
* every aligner form: rendered pairs under a true motion of 0.5 rad about one axis and x = 0.2, started near the truth,
  three fixed iterations, on the smallest sizes that select one wave (40x30), 4 x 256 threads (80x60), 1024 threads
  (160x120), the sliding-window kernel and its exact fall-back (200x194, the first level beyond LDS, batches pinned), the
  exact kernel alone there, and the wide form (160x120, one pair, latency forms): poses within 1e-9 of the oracle, equal
  iteration counts and valid pixels, flags 0 -- but for PHOVO_PAIR_WINDOW_FALLBACK on the sliding-window launch, which is
  predicted on the CPU by the window's restatement (tests/slide_window.py): a rotation of 0.5 rad in the image plane
  leaves the window, and that pair IS the fall-back's case: handed over before its first iteration, it has the bits of
  the exact kernel alone;
* one of these motions at 640x480 with the shipped configuration file (thresholds 300): levels 160x120 and 80x60 in one
  fused launch.

Every alignment reference is held to the well-posedness the flat bar needs (tests/plan_boundaries.py): cond(J^T J) < 1e5
and one ulp of fx moves the oracle's own result by less than a quarter of the bar, with the same iteration counts.
"""
import functools
import os

import numpy as np
import pytest

import edge_states
import plan_boundaries as pb
import slide_window as sw
from test_gpu_pair_system import _check_against, _numpy_system, _oracle_trace_system, _planes

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG4 = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")
POSE_TOL = pb.POSE_TOL
FY_OVER_FX = 1.0625

# ------------------------------------------------------------------------------------------------------------------------
# the row itself
# ------------------------------------------------------------------------------------------------------------------------
ROW_SIZE, ROW_LEVELS = (160, 120), 3
ROW_MOTION = np.array([0.012, -0.009, 0.011, 0.02, -0.015, 0.01])
ANGLES = (0.3, -0.3, 0.8, -0.8, 1.5, -1.5, 2.8, -2.8)
TRIPLES = ((0.3, -0.3, 0.3), (-0.8, 0.3, -0.3), (1.5, 0.3, 0.3), (2.8, -0.3, 0.3), (-0.3, -0.3, 0.8), (0.5, 0.2, -0.4),
           (-1.5, -0.3, -0.3), (-2.8, 0.3, -0.3), (0.3, 2.8, 0.3), (-0.3, 0.3, -2.8), (0.8, -2.8, 0.3), (3.0, 3.0, 3.0))
ROTATIONS = tuple(tuple(a if k == axis else 0.0 for k in range(3)) for axis in range(3) for a in ANGLES) + TRIPLES
TRANSLATIONS = ((0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (-0.3, 0.0, 0.0), (0.0, 0.3, 0.0), (0.0, -0.3, 0.0), (0.0, 0.0, 0.3),
                (0.0, 0.0, -0.3), (0.3, -0.3, 0.3))
# rotation (index into ROTATIONS) -> bit t set: TRANSLATIONS[t] is kept.  Filtered on the CPU: the oracle fills at least a
# quarter of the rows on each of the three levels at the kept states and at none of the others.
# (Gone: pitch and roll alone at +-1.5 and roll at +-0.8 -- the scene leaves the image; at +-2.8 it is back, mirrored, Z < 0.)
ALL_T = 0b11111111
KEPT = {**{r: ALL_T for r in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17, 22, 23, 24, 25, 26, 27, 29, 30, 31, 33, 35)},
        10: 0b00100101, 11: 0b10100011, 32: 0b01111111, 34: 0b01111111}


def all_candidates():
    return [(r, t) for r in range(len(ROTATIONS)) for t in range(len(TRANSLATIONS))]


def state_of(r, t):
    return np.array(TRANSLATIONS[t] + ROTATIONS[r])


def kept_states():
    return [state_of(r, t) for r, t in all_candidates() if KEPT.get(r, 0) >> t & 1]


@functools.lru_cache(maxsize=None)
def row_pair():
    """The plane scene through a camera with fy != fx (as tests/test_gpu_pass_constants.py)."""
    w, h = ROW_SIZE
    K = synthetic.intrinsics(w, h)
    K[1, 1] *= FY_OVER_FX
    scene = synthetic.Scene(93)
    g0, d0 = synthetic.render(scene, np.eye(4), w, h, K, 0.02, hole_seed=186)
    g1, d1 = synthetic.render(scene, se3.eigen_pose(ROW_MOTION), w, h, K, 0.02, hole_seed=187)
    return dict(gray0=g0, depth0=d0, gray1=g1, depth1=d1, K=K)


def enough_rows(rows, level):
    lw, lh = oracle.level_size(ROW_SIZE[0], ROW_SIZE[1], level)
    return 4 * rows >= lw * lh


def test_the_grid_covers_every_axis_and_sign():
    """(no device work: the filtered grid still has what the test is about)"""
    states = kept_states()
    assert len(states) >= 100
    for axis in range(3):
        alone = [s for s in states if s[3 + axis] != 0.0 and np.count_nonzero(s[3:]) == 1]
        assert {abs(s[3 + axis]) for s in alone} >= {0.3, 2.8} and {np.sign(s[3 + axis]) for s in alone} == {1.0, -1.0}
        assert any(s[0] != 0.0 for s in alone) and any(s[1] != 0.0 for s in alone) and any(s[2] != 0.0 for s in alone)
    assert any(abs(s[3]) in (0.8, 1.5) for s in states)
    assert sum(np.count_nonzero(s[3:]) == 3 for s in states) >= 16


@pytest.mark.parametrize("level", range(ROW_LEVELS))
def test_row_matches_the_oracle_at_large_states(level):
    p = row_pair()
    w, h = ROW_SIZE
    states = np.stack(kept_states())
    n = len(states)
    with odometry.AlignmentEngine() as eng:
        eng.set_config(native.make_config(num_levels=ROW_LEVELS, max_iter=[1] * ROW_LEVELS, min_grad=[0.0] * ROW_LEVELS))
        eng.set_build_all_levels(True)
        eng.set_intrinsic_matrix(p["K"])
        eng.reserve_frames(2, w, h)
        eng.upload_frame(0, p["gray0"], p["depth0"])
        eng.upload_frame(1, p["gray1"], p["depth1"])
        planes = _planes(eng, ROW_LEVELS, w, h, range(ROW_LEVELS))
        s = eng.evaluate_pairs([0] * n, [1] * n, states, level)
    worst = 0.0
    for i in range(n):
        rows, _, _ = _oracle_trace_system(planes, level, p["K"], states[i], None)
        assert enough_rows(rows, level), (level, states[i], rows)
        H, g, cost = _numpy_system(planes, level, p["K"], states[i], None)
        worst = max(worst, np.max(np.abs(s["information"][i] - H)) / np.max(np.abs(H)))
        try:
            _check_against(s["information"][i], s["gradient"][i], s["rows"][i], s["cost"][i], H, g, rows, cost)
        except AssertionError as ex:
            raise AssertionError(f"level {level}, state {states[i]}: {ex}") from ex
        assert s["flags"][i] == 0, (level, states[i], s["flags"][i])
    print(f"jacobian row level {level}: {n} states, worst |H - H_ref| / max|H_ref| = {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------------
# every aligner form
# ------------------------------------------------------------------------------------------------------------------------
ITERS = 3
# The true motions: 0.5 rad about one axis at a time with x = 0.2 -- and two more.  The reference pairs the residual
# scattered to target t with row t of J, which is filled only if t is itself a source pixel whose warp stays in the image.
# Half a radian of pitch with x = 0.2 moves every pixel by more than half the image's width and of roll, either way, by more
# than half its height (at the 4:3 sizes): no target is such a pixel, J^T r is exactly zero and the state does not move, whatever the row
# holds (these two still hold the counts, the flags and a finite solve of J^T J).  So the pitch also runs the other way, where
# x = 0.2 works against it, and the roll at 0.3 rad: there, and under the yaw, residuals count (COUNTS, checked below).
MOTIONS = {
    "yaw": (0.2, 0.0, 0.0, 0.5, 0.0, 0.0),
    "pitch": (0.2, 0.0, 0.0, 0.0, 0.5, 0.0),
    "roll": (0.2, 0.0, 0.0, 0.0, 0.0, 0.5),
    "pitch_back": (0.2, 0.0, 0.0, 0.0, -0.5, 0.0),
    "roll_0.3": (0.2, 0.0, 0.0, 0.0, 0.0, 0.3),
}
AXES = list(MOTIONS)
COUNTS = ("yaw", "pitch_back", "roll_0.3")


def axis_motion(axis):
    return list(MOTIONS[AXES[axis]])


# form -> size, what is set on the engine, pairs, the launch kinds, threads of the first launch
FORMS = {
    "one_wave": dict(size=(40, 30), pairs=2, kinds=["persistent"], threads=64),
    "quad_256": dict(size=(80, 60), pairs=2, kinds=["persistent"], threads=256),
    "wide_1024": dict(size=(160, 120), pairs=2, kinds=["persistent"], threads=1024),
    "slide": dict(size=pb.BEYOND, pairs=2, batch_invariant=True, kinds=["slide", "slide_fallback"], threads=sw.SLIDE_THREADS),
    "exact_hbm": dict(size=pb.BEYOND, pairs=2, batch_invariant=True, slide_off=True, kinds=["persistent"], threads=1024),
    "wide_form": dict(size=(160, 120), pairs=1, latency=True, kinds=["wide"], threads=None),
}
assert pb.BEYOND[0] * pb.BEYOND[1] > 38784


@functools.lru_cache(maxsize=None)
def form_pair(size, axis):
    return synthetic.render_pair_with_motion(120 + axis, size[0], size[1], axis_motion(axis))


def _pyramids(ocfg, p):
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    return i0p, d0p, i1p, gxp, gyp


def well_posed(ref):
    assert ref.finite and ref.cond < pb.COND_MAX, ref.cond
    moved, its = ref.nudged()
    assert its == ref.its and moved < 0.25 * POSE_TOL, (moved, its, ref.its)
    return ref


@functools.lru_cache(maxsize=None)
def form_ref(size, axis):
    """The oracle's three iterations on one level of `size`, and the window's verdict on the state entering each."""
    p = form_pair(size, axis)
    _, ocfg = pb.cfgs([ITERS])
    init = p["motion"] + edge_states.NEAR
    planes = _pyramids(ocfg, p)
    ref = well_posed(pb.PhotoRef(ocfg, p["K"], planes, init))
    entering = [init] + [e["state"] for e in ref.trace[:-1]]
    out = [sw.leaves_window(s, p["K"], planes[1][0], size[0], size[1]).leaves for s in entering]
    ref.leaves, ref.leaves_at_once = any(out), out[0]
    return ref


def _upload(eng, p):
    h, w = p["gray0"].shape
    eng.set_intrinsic_matrix(p["K"])
    eng.reserve_frames(2, w, h)
    eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
    eng.upload_frame(1, p["gray1"], None, roles=native.ROLE_TARGET)


def _align(form, p, ncfg, init):
    f = FORMS[form]
    n = f["pairs"]
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        if f.get("batch_invariant"):
            eng.set_batch_invariant(True)
        if f.get("slide_off"):
            eng.set_slide_policy(-1)
        if f.get("latency"):
            eng.set_latency_forms(True)
        _upload(eng, p)
        s, reps = eng.align_pairs([0] * n, [1] * n, init_states=np.tile(init, (n, 1)), want_reports=True)
        launches = eng.last_launches()
    return s, reps, launches


def _check_pose(ref, state, rep, flags, what):
    nl = len(ref.its)
    d = se3.state_distance(state, ref.state)
    print(f"jacobian row {what}: pose distance {d:.3e}, cond {ref.cond:.2e}, valid {ref.valid}, iterations {ref.its}")
    assert list(rep.iterations[:nl]) == ref.its, (what, list(rep.iterations[:nl]), ref.its)
    assert list(rep.valid_pixels[:nl]) == ref.valid, (what, list(rep.valid_pixels[:nl]), ref.valid)
    assert rep.flags == flags, (what, rep.flags, flags)
    assert d <= POSE_TOL, (what, d)


@pytest.mark.parametrize("axis", range(len(AXES)), ids=AXES)
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_matches_the_oracle_under_half_a_radian(form, axis):
    f = FORMS[form]
    size = f["size"]
    p = form_pair(size, axis)
    ref = form_ref(size, axis)
    ncfg, _ = pb.cfgs([ITERS])
    init = p["motion"] + edge_states.NEAR
    s, reps, launches = _align(form, p, ncfg, init)
    kinds = [r["kind"] for r in launches]
    assert kinds[0] == f["kinds"][0] and set(kinds) <= set(f["kinds"]), (form, kinds)
    if f["threads"] is not None:
        assert launches[0]["threads"] == f["threads"], (form, launches[0])
    flags = native.PAIR_WINDOW_FALLBACK if form == "slide" and ref.leaves else 0
    for k in range(f["pairs"]):
        _check_pose(ref, s[k], reps[k], flags, f"{form} {pb.size_id(size)} {AXES[axis]}")
        assert np.array_equal(s[k], s[0])
    if form == "slide" and ref.leaves_at_once:       # every iteration ran in the fall-back: the bits are the exact kernel's
        exact, _, _ = _align("exact_hbm", p, ncfg, init)         # (the two kernels sum a level's pixels in different orders)
        assert np.array_equal(s, exact), (AXES[axis], s, exact)


def test_the_slide_cases_reach_both_kernels():
    """(no device work) Of the three motions at least one stays inside the window for all its iterations -- the
    sliding-window kernel carries the row -- and at least one leaves it: the exact fall-back does."""
    leaves = {name: form_ref(pb.BEYOND, axis).leaves for axis, name in enumerate(AXES)}
    assert any(leaves[name] for name in COUNTS) and not all(leaves[name] for name in COUNTS), leaves
    assert any(form_ref(pb.BEYOND, axis).leaves_at_once for axis in range(len(AXES)))


def test_residuals_count_where_they_are_said_to():
    """(no device work) Under the motions of COUNTS the oracle's gradient is not zero and its state moves in every iteration, on
    every size."""
    for size in sorted({f["size"] for f in FORMS.values()}):
        for axis, name in enumerate(AXES):
            ref = form_ref(size, axis)
            if name in COUNTS:
                assert all(g > 1.0 for _, g in ref.gnorms), (size, name, ref.gnorms)


# ------------------------------------------------------------------------------------------------------------------------
# the shipped thresholds through the fused launch
# ------------------------------------------------------------------------------------------------------------------------
FUSED_AXIS = AXES.index("yaw")


def test_shipped_thresholds_through_the_fused_launch():
    w, h = 640, 480
    p = synthetic.render_pair_with_motion(130, w, h, axis_motion(FUSED_AXIS))
    init = p["motion"] + edge_states.NEAR
    ncfg = native.read_config_file(CFG4)
    nl = ncfg.num_levels
    ocfg = oracle.make_config(num_levels=nl, blur=list(ncfg.blur_filter_size[:nl]),
                              grad_scale=list(ncfg.image_gradients_scaling_factor[:nl]),
                              lam=list(ncfg.lambda_optimization_step[:nl]), max_iter=list(ncfg.max_num_iterations[:nl]),
                              min_grad=list(ncfg.min_gradient_norm[:nl]))
    ref = well_posed(pb.PhotoRef(ocfg, p["K"], _pyramids(ocfg, p), init))
    assert [l for l, _ in ref.gnorms].count(3) >= 2 and [l for l, _ in ref.gnorms].count(2) >= 1, ref.gnorms
    # no gradient norm of the trace within 0.5 % of the threshold (the rule of the fused bases, tests/plan_boundaries.py)
    assert all(abs(g / 300.0 - 1.0) > pb.THRESHOLD_MARGIN for _, g in ref.gnorms), ref.gnorms
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        _upload(eng, p)
        s, reps = eng.align_pairs([0] * 9, [1] * 9, init_states=np.tile(init, (9, 1)), want_reports=True)
        launches = eng.last_launches()
    assert [(r["kind"], r["threads"]) for r in launches] == [("fused", 512)], launches
    for k in range(9):
        _check_pose(ref, s[k], reps[k], 0, f"fused 640x480 {AXES[FUSED_AXIS]} pair {k}")
        assert np.array_equal(s[k], s[0])
