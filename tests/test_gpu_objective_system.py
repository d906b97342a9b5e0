"""GPU tests of phovo_engine_evaluate_objective_pairs / phovo_odometry_get_objective_system: the system of
the trust-region and of the bi-objective aligner at a given state on one level, against the two CPU checkers fed the planes
as the device holds them (tests/objective_system_ref.py), against the aligners' own reports, and then bit identity of the
record, no interference with alignments and with the other evaluate calls, the class surface, the refusals, bad depth and
the flags.  The bars are tests/test_gpu_pair_system.py::_check_against's."""
import ctypes as C

import numpy as np
import pytest

import objective_system_ref as osr

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, synthetic

pytestmark = pytest.mark.gpu

TR, BI = native.OBJECTIVE_TRUST_REGION, native.OBJECTIVE_BIOBJECTIVE
OBJECTIVES = [TR, BI]
OBJECTIVE_IDS = ["trust_region", "biobjective"]
_PAIRS = {}


def _pair(w, h):
    if (w, h) not in _PAIRS:
        _PAIRS[(w, h)] = osr.make_pair(w, h)
    return _PAIRS[(w, h)]


def _upload(e, p):
    h, w = p["gray0"].shape
    e.reserve_frames(2, w, h)
    e.upload_frame(0, p["gray0"], p["depth0"])
    e.upload_frame(1, p["gray1"], p["depth1"])


def _engine(objective, p, nl=1, max_iter=None, upload=True):
    e = odometry.AlignmentEngine(0)
    e.set_config(native.make_config(num_levels=nl, max_iter=max_iter or [1] * nl, min_grad=[0.0] * nl))
    e.set_intrinsic_matrix(p["K"])
    e.set_objective(objective)
    if upload:
        _upload(e, p)
    return e


def _device_planes(e, objective, level=0):
    i0, d0, _, _ = e.get_level_planes(0, level)
    i1, d1, gx, gy = e.get_level_planes(1, level)
    pl = dict(i0=i0, d0=d0, i1=i1, d1=d1, gx=gx, gy=gy)
    if objective == BI:
        pl["dgx"], pl["dgy"] = e.get_level_depth_gradients(1, level)
        pl["gain"] = e.get_level_depth_gain(1, level)
    return pl


def _reference(objective, pl, K, state, lo=0.3, hi=5.0, level=0):
    if objective == TR:
        return osr.trust_region_system(pl["i0"], pl["d0"], pl["i1"], pl["gx"], pl["gy"], level, K, state, lo, hi)
    return osr.biobjective_system(pl["i0"], pl["d0"], pl["i1"], pl["d1"], pl["gx"], pl["gy"], pl["dgx"], pl["dgy"],
                                  pl["gain"], level, K, state, lo, hi)


def _bytes(rec, k=None):
    s = rec["structs"]
    return b"".join(bytes(x) for x in s) if k is None else bytes(s[k])


# ---- 1: checker parity on every directed fixture ------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", osr.SIZES, ids=["%dx%d" % s for s in osr.SIZES])
@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_checker_parity(objective, w, h):
    p = _pair(w, h)
    st = osr.states(p)
    with _engine(objective, p) as e:
        pl = _device_planes(e, objective)
        rec = e.evaluate_objective_pairs([0] * 4, [1] * 4, st, 0)
    for k in range(4):
        ref = _reference(objective, pl, p["K"], st[k])
        print(w, h, "ABCD"[k], "rows", int(rec["rows"][k]), ref["rows"], "cost", float(rec["cost"][k]), ref["cost"])
        osr.check_record(rec, k, ref, relative=ref["rows"] >= 6)
    if (w, h) not in osr.STRIPS:
        assert all(rec["rows"] >= 6) and not rec["flags"].any()


# ---- 2, 3: the aligners' own reports ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,nl", [(160, 120, 2), (200, 152, 1)], ids=["two_levels_160x120", "one_level_200x152"])
def test_trust_region_aligner_cross_check(w, h, nl):
    p = _pair(w, h)
    with _engine(TR, p, nl, [8] * nl) as e:
        x, reps = e.align_pairs([0], [1], want_reports=True)
        tr = e.trust_region_reports(1)
        rec = e.evaluate_objective_pairs([0], [1], x, 0)
    assert tr["steps"][0, 0] > 0
    assert int(rec["rows"][0]) == int(tr["rows"][0, 0])
    final = float(tr["final_cost"][0, 0])
    assert abs(rec["cost"][0] - 2.0 * final) <= 1e-12 * 2.0 * final, (rec["cost"][0], 2.0 * final)
    ref = dict(H=rec["information"][0], cost=float(rec["cost"][0]))
    gn = float(np.linalg.norm(rec["gradient"][0]))
    assert abs(gn - reps[0].gradient_norm) <= osr.gradient_norm_bar(ref), (gn, reps[0].gradient_norm)
    assert rec["flags"][0] == 0


@pytest.mark.parametrize("which", [1, 2], ids=["from_B", "from_C"])
@pytest.mark.parametrize("w,h", [(75, 53), (160, 120)], ids=["75x53", "160x120"])
def test_biobjective_aligner_cross_check(w, h, which):
    p = _pair(w, h)
    start = osr.states(p)[which]
    with _engine(BI, p, 1, [1]) as e:
        _, reps = e.align_pairs([0], [1], init_states=start[None], want_reports=True)
        rec = e.evaluate_objective_pairs([0], [1], start[None], 0)
    assert int(rec["rows"][0]) == int(reps[0].valid_pixels[0])
    ref = dict(H=rec["information"][0], cost=float(rec["cost"][0]))
    gn = float(np.linalg.norm(rec["gradient"][0]))            # (the report is of the system at the initial state)
    assert abs(gn - reps[0].gradient_norm) <= osr.gradient_norm_bar(ref), (gn, reps[0].gradient_norm)


# ---- 4: one arithmetic per pair ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_record_does_not_depend_on_batch_or_settings(objective):
    p = _pair(75, 53)
    st = osr.states(p)
    rs = np.random.RandomState(5)
    batch = p["motion"] + rs.uniform(-0.01, 0.01, (64, 6))
    batch[37] = st[2]
    with _engine(objective, p) as e:
        alone = _bytes(e.evaluate_objective_pairs([0], [1], st[2:3], 0, want_structs=True))
        assert any(alone)
        among = e.evaluate_objective_pairs([0] * 64, [1] * 64, batch, 0, want_structs=True)
        assert _bytes(among, 37) == alone
        for setting in (lambda: e.set_level_fusion(native.FUSION_OFF), lambda: e.set_latency_forms(True),
                        lambda: e.set_batch_invariant(True)):
            setting()
            assert _bytes(e.evaluate_objective_pairs([0], [1], st[2:3], 0, want_structs=True)) == alone


@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_second_owner_group_gives_the_same_record(objective):
    """219 owner maps of 640x480 exceed 256 MB: the call runs in two groups (218 pairs and 1)."""
    p = synthetic.make_pair(31, 640, 480, holes=0.02)
    n = 219
    assert n * 640 * 480 * 4 > (256 << 20) >= (n - 1) * 640 * 480 * 4
    with _engine(objective, p) as e:
        rec = e.evaluate_objective_pairs([0] * n, [1] * n, np.tile(p["motion"], (n, 1)), 0, want_structs=True)
    first = _bytes(rec, 0)
    assert rec["rows"][0] > 100000 and rec["flags"][0] == 0
    assert all(_bytes(rec, k) == first for k in range(n))


# ---- 5: no interference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_evaluate_between_enqueue_and_fetch(objective):
    p = _pair(160, 120)
    st = osr.states(p)

    def run(evaluate):
        with _engine(objective, p, 2, [4, 4]) as e:
            e.enqueue_align([0, 0], [1, 1], init_states=st[:2])
            mid = e.evaluate_objective_pairs([0] * 4, [1] * 4, st, 0, want_structs=True) if evaluate else None
            x, reps = e.fetch_results(2, want_reports=True)
            tr = e.trust_region_reports(2).tobytes() if objective == TR else b""
            return x, b"".join(bytes(r) for r in reps), tr, mid

    x0, r0, t0, _ = run(False)
    x1, r1, t1, mid = run(True)
    assert np.array_equal(x0, x1) and r0 == r1 and t0 == t1
    with _engine(objective, p, 2, [4, 4]) as e:
        assert _bytes(e.evaluate_objective_pairs([0] * 4, [1] * 4, st, 0, want_structs=True)) == _bytes(mid)


def _call_pairs(e, p, n):
    e.set_objective(native.OBJECTIVE_PHOTOMETRIC)
    _upload(e, p)
    e.evaluate_pairs([0] * n, [1] * n, np.tile(p["motion"], (n, 1)), 0)


def _call_sampled(e, p, n):
    e.set_objective(native.OBJECTIVE_PHOTOMETRIC)
    e.set_extensions(native.make_extensions(sampling=native.SAMPLING_BILINEAR))
    _upload(e, p)
    e.evaluate_sampled_pairs([0] * n, [1] * n, np.tile(p["motion"], (n, 1)), 0)
    e.set_extensions(native.make_extensions())


def _call_geometric(e, p, n):
    e.set_objective(native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
    _upload(e, p)
    e.evaluate_geometric_pairs([0] * n, [1] * n, np.tile(p["motion"], (n, 1)), 0)


def _call_other_objective(other):
    def call(e, p, n):
        e.set_objective(other)
        _upload(e, p)
        e.evaluate_objective_pairs([0] * n, [1] * n, np.tile(osr.STATE_C, (n, 1)), 0)
    return call


@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_shares_the_workspace_with_the_other_evaluate_calls(objective):
    """Every evaluate entry point under the objective it serves, then this one: the bytes of a fresh engine.  The earlier
    call is made with more pairs and with fewer than the later one, so the watermark of owner maps known to hold -1 is
    crossed in both directions (a larger area behind a smaller one holds the earlier call's ballots and sums)."""
    p = _pair(75, 53)
    st = osr.states(p)
    with _engine(objective, p) as e:
        fresh = _bytes(e.evaluate_objective_pairs([0] * 4, [1] * 4, st, 0, want_structs=True))
    other = BI if objective == TR else TR
    for before in (_call_pairs, _call_sampled, _call_geometric, _call_other_objective(other)):
        for n_before in (1, 9):
            with _engine(objective, p, upload=False) as e:
                before(e, p, n_before)
                e.set_objective(objective)
                _upload(e, p)
                got = _bytes(e.evaluate_objective_pairs([0] * 4, [1] * 4, st, 0, want_structs=True))
                assert got == fresh, (before.__name__, n_before)
                before(e, p, n_before)
                e.set_objective(objective)
                _upload(e, p)
                assert _bytes(e.evaluate_objective_pairs([0] * 4, [1] * 4, st, 0, want_structs=True)) == fresh


# ---- 6: the class surface ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_class_surface_and_not_ready(objective):
    p = _pair(160, 120)
    cls = odometry.CPhotoconsistencyOdometryCeres if objective == TR else odometry.CPhotoconsistencyOdometryBiObjective
    cfg = native.make_config(num_levels=3, max_iter=[0, 3, 3], min_grad=[0.0] * 3)      # finest optimised level: 1
    with cls(0) as od:
        od.SetConfiguration(cfg)
        od.SetIntrinsicMatrix(p["K"])
        od.SetSourceFrame(p["gray0"], p["depth0"])
        od.SetTargetFrame(p["gray1"], p["depth1"])
        od.SetInitialStateVector(np.zeros(6))
        with pytest.raises(native.PhovoError) as ei:
            od.GetObjectiveSystem()
        assert ei.value.status == native.E_NOT_READY
        od.Optimize()
        ps = od.GetObjectiveSystem()
        raw = native.PairSystem()
        assert od._lib.phovo_odometry_get_objective_system(od._h, C.byref(raw)) == native.OK
        assert bytes(raw) == bytes(ps)
        assert od._lib.phovo_odometry_get_objective_system(od._h, None) == native.E_INVALID_ARGUMENT
        assert od._lib.phovo_odometry_get_objective_system(None, C.byref(raw)) == native.E_INVALID_ARGUMENT
        state = od.GetOptimalStateVector()
        od.SetSourceFrame(p["gray0"], p["depth0"])
        with pytest.raises(native.PhovoError) as ei:
            od.GetObjectiveSystem()
        assert ei.value.status == native.E_NOT_READY
        od.SetSourceFrame(p["gray0"], p["depth0"])
        od.Optimize()
        od.SetTargetFrame(p["gray1"], p["depth1"])
        with pytest.raises(native.PhovoError) as ei:
            od.GetObjectiveSystem()
        assert ei.value.status == native.E_NOT_READY
    e = odometry.AlignmentEngine(0)
    with e:
        e.set_config(cfg)
        e.set_intrinsic_matrix(p["K"])
        e.set_objective(objective)
        _upload(e, p)
        rec = e.evaluate_objective_pairs([0], [1], state[None], 1, want_structs=True)
    assert _bytes(rec) == bytes(ps) and ps.rows >= 6


def test_class_call_is_unsupported_under_the_other_objectives():
    p = _pair(75, 53)
    for cls in (odometry.CPhotoconsistencyOdometryAnalytic, odometry.CPhotoconsistencyOdometryAffine,
                odometry.CPhotoconsistencyOdometryGeometric):
        with cls(0) as od:
            assert not hasattr(od, "GetObjectiveSystem")
            raw = native.PairSystem()
            assert od._lib.phovo_odometry_get_objective_system(od._h, C.byref(raw)) == native.E_UNSUPPORTED


# ---- 7: refusals ------------------------------------------------------------------------------------------------------
def _raw(e, n, src, tgt, states, level, out):
    ip = C.POINTER(C.c_int)
    return e._lib.phovo_engine_evaluate_objective_pairs(
        e._h, n, None if src is None else src.ctypes.data_as(ip), None if tgt is None else tgt.ctypes.data_as(ip),
        None if states is None else states.ctypes.data, level, None if out is None else out.ctypes.data)


@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_refusals(objective):
    p = _pair(75, 53)
    src, tgt = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    st = np.zeros((1, 6))
    out = np.zeros(1, dtype=odometry.PAIR_SYSTEM_DTYPE)
    lib = native.lib()
    assert lib.phovo_engine_evaluate_objective_pairs(None, 1, src.ctypes.data_as(C.POINTER(C.c_int)),
                                                     tgt.ctypes.data_as(C.POINTER(C.c_int)), st.ctypes.data, 0,
                                                     out.ctypes.data) == native.E_INVALID_ARGUMENT
    with _engine(objective, p, 2, [1, 0]) as e:                       # level 1 is not optimised: not stored
        assert _raw(e, 1, src, tgt, st, 0, out) == native.OK
        assert _raw(e, 1, None, tgt, st, 0, out) == native.E_INVALID_ARGUMENT
        assert _raw(e, 1, src, None, st, 0, out) == native.E_INVALID_ARGUMENT
        assert _raw(e, 1, src, tgt, None, 0, out) == native.E_INVALID_ARGUMENT
        assert _raw(e, 1, src, tgt, st, 0, None) == native.E_INVALID_ARGUMENT
        assert _raw(e, -1, src, tgt, st, 0, out) == native.E_INVALID_ARGUMENT
        assert _raw(e, 0, None, None, None, 0, None) == native.OK
        assert _raw(e, 0, None, None, None, 2, None) == native.E_INVALID_ARGUMENT
        assert _raw(e, 1, src, tgt, st, -1, out) == native.E_INVALID_ARGUMENT
        assert _raw(e, 1, src, tgt, st, 2, out) == native.E_INVALID_ARGUMENT
        assert not e.level_is_stored(1)
        assert _raw(e, 1, src, tgt, st, 1, out) == native.E_NOT_READY
        for bad in (-1, 2):
            assert _raw(e, 1, np.array([bad], dtype=np.int32), tgt, st, 0, out) == native.E_INVALID_ARGUMENT
            assert _raw(e, 1, src, np.array([bad], dtype=np.int32), st, 0, out) == native.E_INVALID_ARGUMENT
    with _engine(objective, p, upload=False) as e:                    # roles
        assert _raw(e, 1, src, tgt, st, 0, out) == native.E_NOT_READY            # no frames
        e.reserve_frames(2, 75, 53)
        e.upload_frame(0, p["gray0"], p["depth0"], native.ROLE_SOURCE)
        e.upload_frame(1, p["gray1"], p["depth1"], native.ROLE_TARGET)
        assert _raw(e, 1, src, tgt, st, 0, out) == native.OK
        assert _raw(e, 1, tgt, tgt, st, 0, out) == native.E_NOT_READY            # frame 1 has no source role
        assert _raw(e, 1, src, src, st, 0, out) == native.E_NOT_READY            # frame 0 has no target role


@pytest.mark.parametrize("other", [native.OBJECTIVE_PHOTOMETRIC, native.OBJECTIVE_PHOTOMETRIC_AFFINE,
                                   native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC], ids=["photometric", "affine", "geometric"])
def test_other_objectives_are_unsupported_and_named_their_call(other):
    p = _pair(75, 53)
    serves = {native.OBJECTIVE_PHOTOMETRIC: "phovo_engine_evaluate_pairs",
              native.OBJECTIVE_PHOTOMETRIC_AFFINE: "phovo_engine_evaluate_sampled_pairs",
              native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC: "phovo_engine_evaluate_geometric_pairs"}[other]
    with _engine(other, p) as e:
        with pytest.raises(native.PhovoError) as ei:
            e.evaluate_objective_pairs([0], [1], np.zeros((1, 6)), 0)
        assert ei.value.status == native.E_UNSUPPORTED and serves in str(ei.value)
        with pytest.raises(native.PhovoError) as ei:                 # before anything about the call is looked at
            e.evaluate_objective_pairs([], [], np.zeros((0, 6)), 7)
        assert ei.value.status == native.E_UNSUPPORTED


# ---- 8: bad depth and the flags -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_bad_source_depth_and_gate_bounds(objective):
    p = dict(_pair(75, 53))
    d = p["depth0"].copy()
    d[5, :] = np.nan
    d[:, 7] = np.inf
    d[11, :] = 0.3                      # exactly at both bounds of the gate: excluded
    d[:, 13] = 5.0
    p["depth0"] = d
    st = osr.states(p)
    with _engine(objective, p) as e:
        pl = _device_planes(e, objective)
        assert np.isnan(pl["d0"][5, 0]) and np.isinf(pl["d0"][0, 7]) and pl["d0"][11, 0] == 0.3 and pl["d0"][0, 13] == 5.0
        rec = e.evaluate_objective_pairs([0] * 4, [1] * 4, st, 0)
    for k in range(4):
        ref = _reference(objective, pl, p["K"], st[k])
        assert ref["rows"] >= 6 and ref["flags"] == 0
        osr.check_record(rec, k, ref)


@pytest.mark.parametrize("objective", OBJECTIVES, ids=OBJECTIVE_IDS)
def test_no_landing_pixel_and_nan_state(objective):
    p = _pair(75, 53)
    away = np.array([50.0, 0.0, 0.0, 0.0, 0.0, 0.0])                 # every pixel projects far outside the image
    nan = np.array([0.0, np.nan, 0.0, 0.0, 0.0, 0.0])
    with _engine(objective, p) as e:
        rec = e.evaluate_objective_pairs([0, 0], [1, 1], np.stack([away, nan]), 0)
    for k in range(2):
        assert rec["rows"][k] == 0 and rec["flags"][k] == native.PAIR_RANK_DEFICIENT
        assert not rec["information"][k].any() and not rec["gradient"][k].any() and rec["cost"][k] == 0.0
