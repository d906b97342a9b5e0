"""How the level kernels' two passes get their constants (run with -m gpu on an MI355X).

Wave 0 writes the constant block in the order the passes consume it (write_pass_constants, csrc/gn_device.hpp): the two
projected rows of Rt and the translation already multiplied by fx / fy, the two unprojection offsets of the level, then
what pass 2 reads.  Pass 1 takes the rotation entries as scalars and the translation and offsets as lane-uniform values
in vector registers, pass 2 its part as scalars.  What can go wrong is a slot read where another one was written, a
product formed with the wrong focal length, a block that is stale or half written when a workgroup goes from one pair
to the next, and focal products that outlive a change of the intrinsic matrix.  So:

* every geometry level_body is compiled for (SOLO, QUAD, MID, WIDE, HUGE with its owner map in HBM, a fused run of two
  levels) aligns one pair at the form's first size of tests/plan_boundaries.py for three iterations against the oracle,
  from an initial state and under a true motion of about 0.1 rad on every axis -- none of the block's constants is
  trivially 0 or 1 -- with fy != fx, at the bar of the other GPU tests (1e-9 on the pose distance, equal iteration counts
  and valid pixels);
* the Huber, fp32 and fp16 instantiations do the same at the QUAD size against the identically extended oracle on the
  planes the device holds (as tests/test_gpu_extensions.py);
* 64 pairs with 64 initial states in one enqueue equal the same pairs one per enqueue bit for bit -- and, because a launch
  has as many workgroups as pairs up to what the chip holds, so that 64 pairs are 64 workgroups of one pair each, the same
  64 states repeated until there are more pairs than workgroups: every workgroup then carries its block from one pair
  into the next;
* after set_intrinsic_matrix on resident frames the result is a fresh engine's, bit for bit.

Every reference is checked to be well-posed for the flat bar: cond(J^T J) < 1e5 and one ulp of fx moves the oracle's own
result by less than a quarter of it (the rules of tests/plan_boundaries.py).
"""
import functools

import numpy as np
import pytest

import plan_boundaries as pb

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

POSE_TOL = pb.POSE_TOL                 # 1e-9, the bar of tests/test_gpu_parity.py
ITERS = 3
FY_OVER_FX = 1.0625
MOTION = np.array([0.012, -0.009, 0.011, 0.10, -0.09, 0.11])          # T_10 of every pair: x, y, z, yaw, pitch, roll
INIT = MOTION + np.array([0.004, -0.003, 0.005, 0.004, 0.005, -0.004])
HUBER_DELTA = 0.05

# the form's first size in tests/plan_boundaries.py (SOLO has no smaller neighbour: 40x30, the 5-level file's coarsest level)
GEOMETRIES = {
    "SOLO": ((40, 30), 64),
    "QUAD": ((50, 41), 256),
    "MID": ((97, 99), 512),
    "WIDE": ((134, 96), 1024),
    "HUGE": (pb.BEYOND, 1024),
}
FUSED_BASE = (200, 164)                # levels 1 and 2: 100x82 and 50x41, the smallest level in the first fusable chunk
FUSED_MAX_ITER, FUSED_MIN_GRAD = [0, ITERS, ITERS], [0.0, 1e-9, 1e-9]        # thresholds set, none reached


def _intrinsics(w, h):
    K = synthetic.intrinsics(w, h)
    K[1, 1] *= FY_OVER_FX
    return K


@functools.lru_cache(maxsize=None)
def _pair(w, h):
    """The plane scene of the other tests seen through a camera with fy != fx, under MOTION."""
    scene = synthetic.Scene(91)
    K = _intrinsics(w, h)
    g0, d0 = synthetic.render(scene, np.eye(4), w, h, K, 0.02, hole_seed=182)
    g1, d1 = synthetic.render(scene, se3.eigen_pose(MOTION), w, h, K, 0.02, hole_seed=183)
    return dict(gray0=g0, depth0=d0, gray1=g1, depth1=d1, K=K)


def _pyramids(ocfg, p):
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    return i0p, d0p, i1p, gxp, gyp


def _reference(ocfg, K, planes, init, huber=None):
    """The oracle's result (pb.PhotoRef), held to the well-posedness the flat bar needs."""
    ref = pb.PhotoRef(ocfg, K, planes, init, huber)
    assert ref.finite and ref.cond < pb.COND_MAX, ref.cond
    moved, its = ref.nudged()
    assert its == ref.its and moved < 0.25 * POSE_TOL, (moved, its, ref.its)
    return ref


@functools.lru_cache(maxsize=None)
def _level_ref(size):
    _, ocfg = pb.cfgs([ITERS])
    p = _pair(*size)
    return _reference(ocfg, p["K"], _pyramids(ocfg, p), INIT)


def _engine(ncfg, p, ext=None):
    h, w = p["gray0"].shape
    e = odometry.AlignmentEngine(0)
    if ext is not None:
        e.set_extensions(ext)
    e.set_config(ncfg)
    e.set_intrinsic_matrix(p["K"])
    e.reserve_frames(2, w, h)
    e.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
    e.upload_frame(1, p["gray1"], None, roles=native.ROLE_TARGET)
    return e


def _align(e, inits):
    inits = np.atleast_2d(np.asarray(inits, dtype=np.float64))
    n = len(inits)
    return e.align_pairs([0] * n, [1] * n, init_states=inits, want_reports=True)


def _check(ref, state, rep, what):
    nl = len(ref.its)
    d = se3.state_distance(state, ref.state)
    print(f"pass constants {what}: pose distance {d:.3e}, cond {ref.cond:.2e}, valid {ref.valid}")
    assert list(rep.iterations[:nl]) == ref.its, (what, list(rep.iterations[:nl]), ref.its)
    assert list(rep.valid_pixels[:nl]) == ref.valid, (what, list(rep.valid_pixels[:nl]), ref.valid)
    assert rep.flags == 0, (what, rep.flags)
    assert abs(rep.gradient_norm - ref.gnorm) <= pb.GRAD_TOL * max(1.0, ref.gnorm), (what, rep.gradient_norm, ref.gnorm)
    assert d < POSE_TOL, (what, d)


# ------------------------------------------------------------------------------------------------------------------------
# oracle parity per geometry
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(GEOMETRIES))
def test_every_geometry_matches_the_oracle(form):
    size, threads = GEOMETRIES[form]
    p = _pair(*size)
    plan = pb.plan_level(size[0] * size[1])
    assert (plan["form"], plan["threads"]) == (form, threads), plan
    assert plan["owner_in_lds"] == (form != "HUGE")
    ncfg, _ = pb.cfgs([ITERS])
    with _engine(ncfg, p) as e:
        if form == "HUGE":                       # the exact kernel alone, its owner map in HBM behind the LDS part
            e.set_wide_policy(-1)
            e.set_slide_policy(-1)
        states, reps = _align(e, INIT)
        launches = [(r["kind"], r["threads"], r["lds_bytes"]) for r in e.last_launches()]
    assert launches == [("persistent", threads, plan["lds_bytes"])], (form, launches)
    _check(_level_ref(size), states[0], reps[0], f"{form} {pb.size_id(size)}")


def test_fused_run_of_two_levels_matches_the_oracle():
    p = _pair(*FUSED_BASE)
    ncfg, ocfg = pb.cfgs(FUSED_MAX_ITER, FUSED_MIN_GRAD)
    ref = _reference(ocfg, p["K"], _pyramids(ocfg, p), INIT)
    assert ref.its[1:] == FUSED_MAX_ITER[1:]             # no threshold ended a level early
    with _engine(ncfg, p) as e:
        assert e.level_size(1) == (100, 82) and e.level_size(2) == (50, 41)
        states, reps = _align(e, INIT)
        kinds = [(r["kind"], r["threads"]) for r in e.last_launches()]
    assert kinds == [("fused", 512)], kinds
    _check(ref, states[0], reps[0], f"fused {pb.size_id(FUSED_BASE)}")


# ------------------------------------------------------------------------------------------------------------------------
# the other instantiations, at the QUAD size
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,storage,huber", [("huber", native.STORAGE_F64, True), ("fp32", native.STORAGE_F32, False),
                                                ("fp16", native.STORAGE_F16, False)])
def test_huber_and_narrow_planes_match_the_extended_oracle(name, storage, huber):
    size, threads = GEOMETRIES["QUAD"]
    p = _pair(*size)
    ncfg, ocfg = pb.cfgs([ITERS])
    ext = native.make_extensions(plane_storage=storage, huber_delta=[HUBER_DELTA] if huber else None)
    with _engine(ncfg, p, ext=ext) as e:
        i0, d0, _, _ = e.get_level_planes(0, 0)          # the planes the device holds, rounded to the storage type
        i1, _, gx, gy = e.get_level_planes(1, 0)
        states, reps = _align(e, INIT)
        kinds = [(r["kind"], r["threads"]) for r in e.last_launches()]
    assert kinds == [("persistent", threads)], kinds
    ref = _reference(ocfg, p["K"], ([i0], [d0], [i1], [gx], [gy]), INIT, [HUBER_DELTA] if huber else None)
    if huber:                                            # the weights are at work: the plain result is another one
        assert se3.state_distance(ref.state, _level_ref(size).state) > 1e-7
    _check(ref, states[0], reps[0], f"QUAD {name} {pb.size_id(size)}")


# ------------------------------------------------------------------------------------------------------------------------
# a workgroup's block from one pair to the next
# ------------------------------------------------------------------------------------------------------------------------
def _sixty_four_states():
    rs = np.random.RandomState(808)
    return INIT + rs.uniform(-1.0, 1.0, (64, 6)) * np.array([0.01, 0.01, 0.01, 0.03, 0.03, 0.03])


def _bits(states, reps):
    return (states.copy(), [int(r.iterations[0]) for r in reps], [int(r.valid_pixels[0]) for r in reps],
            np.array([r.gradient_norm for r in reps]))


def _same_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), what                  # (array_equal: NaN nowhere, the states are finite)
    assert a[1] == b[1] and a[2] == b[2], what
    assert np.array_equal(a[3], b[3]), what


@pytest.mark.parametrize("form,repeats", [("QUAD", 40), ("WIDE", 10)])
def test_no_constant_of_one_pair_reaches_the_next(form, repeats):
    """64 states in one enqueue, the 64 states `repeats` times over in one enqueue (more pairs than the chip holds
    workgroups of this form: each workgroup draws several), and one state per enqueue: the same bits."""
    size, threads = GEOMETRIES[form]
    p = _pair(*size)
    ncfg, _ = pb.cfgs([ITERS])
    inits = _sixty_four_states()
    with _engine(ncfg, p) as e:
        together = _bits(*_align(e, inits))
        assert e.last_launches()[0]["threads"] == threads
        many_inits = np.tile(inits, (repeats, 1))
        s, r = _align(e, many_inits)
        workgroups = e.last_launches()[0]["workgroups"]
        alone = [_align(e, st) for st in inits]
    assert np.all(np.isfinite(together[0])) and len({st.tobytes() for st in together[0]}) == 64
    assert 2 * workgroups <= len(many_inits), (workgroups, len(many_inits))       # at least two pairs per workgroup
    one_by_one = _bits(np.stack([a[0][0] for a in alone]), [a[1][0] for a in alone])
    _same_bits(together, one_by_one, f"{form}: 64 pairs in one enqueue against one per enqueue")
    for k in range(repeats):
        _same_bits(_bits(s[64 * k:64 * (k + 1)], r[64 * k:64 * (k + 1)]), one_by_one,
                   f"{form}: copy {k} of the 64 states among {len(many_inits)} pairs on {workgroups} workgroups")


# ------------------------------------------------------------------------------------------------------------------------
# the focal products follow the intrinsic matrix
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["QUAD", "WIDE"])
def test_focal_products_follow_set_intrinsic_matrix(form):
    size, threads = GEOMETRIES[form]
    p = _pair(*size)
    ncfg, _ = pb.cfgs([ITERS])
    K2 = p["K"].copy()
    K2[0, 0] *= 1.03
    K2[1, 1] *= 0.96
    with _engine(ncfg, p) as e:
        first = _bits(*_align(e, INIT))
        e.set_intrinsic_matrix(K2)                           # the frames stay resident
        second = _bits(*_align(e, INIT))
        assert e.last_launches()[0]["threads"] == threads
    with _engine(ncfg, dict(p, K=K2)) as e:
        fresh = _bits(*_align(e, INIT))
    _same_bits(second, fresh, f"{form}: after set_intrinsic_matrix against a fresh engine")
    assert not np.array_equal(first[0], second[0])            # and the change of fx, fy did change the result
