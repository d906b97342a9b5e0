"""GPU tests of the bi-objective aligner (PHOVO_OBJECTIVE_BIOBJECTIVE, gn_biobjective_kernel.hip) against the CPU checker
tests/biobjective_ref.py: target planes bit for bit, poses within 1e-9 with equal iteration and contributing-pixel
counts, the row-collision branches on the device, one arithmetic per pair, no change to the photometric objective, and
the refusals."""
import os

import numpy as np
import pytest

import biobjective_ref as ref

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config_files")
POSE_TOL = 1e-9


def _cfg_file(name, max_iter=None, min_grad=None):
    n = native.read_config_file(os.path.join(CFG, name))
    nl = n.num_levels
    mi = list(n.max_num_iterations[:nl]) if max_iter is None else max_iter
    mg = list(n.min_gradient_norm[:nl]) if min_grad is None else min_grad
    kw = dict(num_levels=nl, blur=list(n.blur_filter_size[:nl]), grad_scale=list(n.image_gradients_scaling_factor[:nl]),
              lam=list(n.lambda_optimization_step[:nl]), max_iter=mi, min_grad=mg)
    return native.make_config(**kw), oracle.make_config(**kw)


@pytest.fixture(scope="module")
def pairs():
    return [synthetic.make_pair(s, 640, 480, holes=0.05 if s % 2 else 0.0) for s in range(3)]


def _engine(ncfg, K, build_all=False):
    e = odometry.AlignmentEngine(0)
    e.set_config(ncfg)
    e.set_intrinsic_matrix(K)
    e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
    if build_all:
        e.set_build_all_levels(True)
    return e


def _upload_pairs(e, ps):
    e.reserve_frames(2 * len(ps), 640, 480)
    for k, p in enumerate(ps):
        e.upload_frame(2 * k, p["gray0"], p["depth0"], native.ROLE_SOURCE)
        e.upload_frame(2 * k + 1, p["gray1"], p["depth1"], native.ROLE_TARGET)


@pytest.mark.parametrize("build_all", [False, True])
def test_target_planes_bit_identical(pairs, build_all):
    ncfg, ocfg = _cfg_file("config_4_level_optimization_analytic.yml")
    p = pairs[1]
    with _engine(ncfg, p["K"], build_all) as e:
        _upload_pairs(e, [p])
        tp = ref.target_planes(p["gray1"], p["depth1"], ocfg, 5.0)
        for level in range(ocfg.num_levels):
            if not e.level_is_stored(level):
                continue
            _, d, _, _ = e.get_level_planes(1, level)
            assert np.array_equal(d, tp["d1"][level]), level
            gx, gy = e.get_level_depth_gradients(1, level)
            ogx, ogy = oracle.scharr(tp["d1"][level] * (1.0 / 5.0), ocfg.image_gradients_scaling_factor[level])
            assert np.array_equal(gx, ogx) and np.array_equal(gy, ogy), level
            gain = e.get_level_depth_gain(1, level)
            assert abs(gain - tp["gain"][level]) <= 1e-14 * abs(tp["gain"][level]), level
        # a later max depth changes the gate, not the planes built at upload
        e.set_depth_range(0.3, 3.0)
        gx2, _ = e.get_level_depth_gradients(1, 3)
        assert np.array_equal(gx2, oracle.scharr(tp["d1"][3] * (1.0 / 5.0), ocfg.image_gradients_scaling_factor[3])[0])


def _check_parity(e, ocfg, ps, init=None):
    n = len(ps)
    states, reps = e.align_pairs(np.arange(n) * 2, np.arange(n) * 2 + 1, init, want_reports=True)
    for k, p in enumerate(ps):
        es, its, valid, flags, _ = ref.align(ocfg, p["K"], p["gray0"], p["depth0"], p["gray1"], p["depth1"],
                                             None if init is None else init[k])
        nl = ocfg.num_levels
        assert list(reps[k].iterations[:nl]) == its, (k, list(reps[k].iterations[:nl]), its)
        assert list(reps[k].valid_pixels[:nl]) == valid, (k, list(reps[k].valid_pixels[:nl]), valid)
        assert se3.state_distance(states[k], es) < POSE_TOL, (k, se3.state_distance(states[k], es))
    return states, reps


@pytest.mark.parametrize("name,max_iter,min_grad", [
    ("config_4_level_optimization_analytic.yml", None, None),
    ("config_4_level_optimization_analytic.yml", [0, 0, 20, 50], [0, 0, 0, 0]),
    ("config_5_level_optimization_analytic.yml", None, None),
    ("config_only_level_0_analytic.yml", [5, 0, 0, 0], None),          # the owner map in HBM
])
def test_parity_with_checker(pairs, name, max_iter, min_grad):
    ncfg, ocfg = _cfg_file(name, max_iter, min_grad)
    ps = pairs[:2] if name.startswith("config_only") else pairs
    with _engine(ncfg, ps[0]["K"]) as e:
        _upload_pairs(e, ps)
        _check_parity(e, ocfg, ps)
        assert {r["kind"] for r in e.last_launches()} == {"biobjective"}


def test_parity_in_the_512_thread_lds_geometry():
    """200x150 at level 0: the owner map (120 kB) exceeds half of LDS but fits it: 512 threads, one workgroup per CU."""
    ps = [synthetic.make_pair(s, 200, 150, holes=0.03) for s in (21, 22)]
    ncfg, ocfg = _cfg_file("config_only_level_0_analytic.yml", [8, 0, 0, 0], [0, 0, 0, 0])
    with _engine(ncfg, ps[0]["K"]) as e:
        e.reserve_frames(4, 200, 150)
        for k, p in enumerate(ps):
            e.upload_frame(2 * k, p["gray0"], p["depth0"], native.ROLE_SOURCE)
            e.upload_frame(2 * k + 1, p["gray1"], p["depth1"], native.ROLE_TARGET)
        _check_parity(e, ocfg, ps)
        assert [(r["kind"], r["threads"]) for r in e.last_launches()] == [("biobjective", 512)]


def test_collision_branches_on_device():
    """A zoom (z translation) with pixel 0 valid: the checker's counters show depth-won rows below N and the row-0 tie."""
    p = synthetic.make_pair(11, 640, 480)
    p["depth0"][0, 0] = 1.0
    ncfg, ocfg = _cfg_file("config_4_level_optimization_analytic.yml", [0, 0, 20, 50], [0, 0, 0, 0])
    init = np.array([[0.0, 0.0, -0.25, 0.0, 0.0, 0.0]])
    _, _, _, _, trace = ref.align(ocfg, p["K"], p["gray0"], p["depth0"], p["gray1"], p["depth1"], init[0])
    assert sum(t["depth_won_below_n"] for t in trace) > 0
    assert sum(t["row0_tie"] for t in trace) > 0
    assert sum(t["depth_rows_at_n"] for t in trace) > 0
    with _engine(ncfg, p["K"]) as e:
        _upload_pairs(e, [p])
        _check_parity(e, ocfg, [p], init)


def test_one_arithmetic_per_pair(pairs):
    ncfg, ocfg = _cfg_file("config_4_level_optimization_analytic.yml", [0, 0, 20, 50], [0, 0, 0, 0])
    p = pairs[0]
    with odometry.CPhotoconsistencyOdometryBiObjective(0) as po:
        po.SetConfiguration(ncfg)
        po.SetIntrinsicMatrix(p["K"])
        po.SetSourceFrame(p["gray0"], p["depth0"])
        po.SetTargetFrame(p["gray1"], p["depth1"])
        po.SetInitialStateVector(np.zeros(6))
        po.Optimize()
        single = po.GetOptimalStateVector()
    with _engine(ncfg, p["K"]) as e:
        _upload_pairs(e, pairs)
        # 512 pairs with pair 0 among them
        rs = np.random.RandomState(1)
        src = rs.randint(0, len(pairs), 512) * 2
        src[137] = 0
        tgt = src + 1
        out = e.align_pairs(src, tgt)
        assert np.array_equal(out[137], single)
    # 8192 pairs from 1024 distinct (source, target) frame combinations of one 32-frame sequence: every copy bit-identical
    seq = synthetic.make_sequence(seed=7, n_frames=32, holes=0.01, workers=8)
    nf = 32
    with _engine(ncfg, seq["K"]) as e:
        e.reserve_frames(nf, 640, 480)
        e.upload_frames(0, seq["gray"], seq["depth"])
        combos = np.array([(a, b) for a in range(nf) for b in range(nf)])
        assert len(combos) == 1024
        idx = np.random.RandomState(2).randint(0, len(combos), 8192)
        idx[:len(combos)] = np.arange(len(combos))
        out = e.align_pairs(combos[idx, 0], combos[idx, 1])
        for c in range(len(combos)):
            same = out[idx == c]
            assert all(np.array_equal(x, same[0], equal_nan=True) for x in same), c


def test_photometric_objective_unchanged_after_switches(pairs):
    ncfg, _ = _cfg_file("config_4_level_optimization_analytic.yml")
    p = pairs[0]

    def run(e):
        e.reserve_frames(2, 640, 480)
        e.upload_frame(0, p["gray0"], p["depth0"], native.ROLE_SOURCE)
        e.upload_frame(1, p["gray1"], None, native.ROLE_TARGET)
        return e.align_pairs([0], [1])

    with odometry.AlignmentEngine(0) as fresh:
        fresh.set_config(ncfg)
        fresh.set_intrinsic_matrix(p["K"])
        base = run(fresh)
    with odometry.AlignmentEngine(0) as e:
        e.set_config(ncfg)
        e.set_intrinsic_matrix(p["K"])
        run(e)
        e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
        assert e.get_objective() == native.OBJECTIVE_BIOBJECTIVE
        with pytest.raises(native.PhovoError) as ei:           # the pool was dropped
            e.align_pairs([0], [1])
        assert ei.value.status == native.E_NOT_READY
        e.reserve_frames(2, 640, 480)
        e.upload_frame(0, p["gray0"], p["depth0"], native.ROLE_SOURCE)
        e.upload_frame(1, p["gray1"], p["depth1"], native.ROLE_TARGET)
        e.align_pairs([0], [1])
        e.set_objective(native.OBJECTIVE_PHOTOMETRIC)
        with pytest.raises(native.PhovoError) as ei:
            e.align_pairs([0], [1])
        assert ei.value.status == native.E_NOT_READY
        assert np.array_equal(run(e), base)


def test_refusals(pairs):
    p = pairs[0]
    unsupported = [native.make_extensions(plane_storage=native.STORAGE_F32),
                   native.make_extensions(plane_storage=native.STORAGE_F16),
                   native.make_extensions(sampling=native.SAMPLING_BILINEAR),
                   native.make_extensions(huber_delta=[0.1] * 4)]
    for ext in unsupported:
        with odometry.AlignmentEngine(0) as e:            # extensions first, objective second
            e.set_extensions(ext)
            with pytest.raises(native.PhovoError) as ei:
                e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
            assert ei.value.status == native.E_UNSUPPORTED
            assert e.get_objective() == native.OBJECTIVE_PHOTOMETRIC
        with odometry.AlignmentEngine(0) as e:            # objective first, extensions second
            e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
            with pytest.raises(native.PhovoError) as ei:
                e.set_extensions(ext)
            assert ei.value.status == native.E_UNSUPPORTED
    ncfg, ocfg = _cfg_file("config_4_level_optimization_analytic.yml")
    with _engine(ncfg, p["K"]) as e:
        e.reserve_frames(2, 640, 480)
        with pytest.raises(native.PhovoError) as ei:
            e.upload_frame(1, p["gray1"], None, native.ROLE_TARGET)
        assert ei.value.status == native.E_INVALID_ARGUMENT
    with odometry.CPhotoconsistencyOdometryBiObjective(0) as po:
        po.SetConfiguration(ncfg)
        with pytest.raises(ValueError):
            po.SetTargetFrame(p["gray1"], None)
    # NaN in the target depth: NaN gain, flagged as the checker predicts
    d1 = p["depth1"].copy()
    d1[8:40, 8:40] = np.nan
    _, _, _, flags, _ = ref.align(ocfg, p["K"], p["gray0"], p["depth0"], p["gray1"], d1)
    assert flags & native.PAIR_NONFINITE
    with _engine(ncfg, p["K"]) as e:
        e.reserve_frames(2, 640, 480)
        e.upload_frame(0, p["gray0"], p["depth0"], native.ROLE_SOURCE)
        e.upload_frame(1, p["gray1"], d1, native.ROLE_TARGET)
        _, reps = e.align_pairs([0], [1], want_reports=True)
        assert reps[0].flags & native.PAIR_NONFINITE
        assert not e.level_uses_wide(3, 1)
