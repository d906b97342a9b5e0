"""phovo_engine_evaluate_inverse_pairs and phovo_odometry_get_inverse_system on the device: the twist-basis
system of the inverse-compositional objective against the numpy checker (tests/inverse_system_ref.py) fed the planes exactly
as the device holds them (get_level_planes), never the code under test.  The bars are the project's own
(sampled_system_ref.check_against): H within 1e-10 of its scale, g within 1e-9 sqrt(H_ii cost), cost within 1e-12 relative,
rows and flags exact.  The fixtures are tests/inverse_system_cases.py's; tests/test_inverse_system_cpu.py holds them to what
this file relies on without a device."""
import ctypes as C

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

import inverse_edges as ie
import inverse_ref as ir
import inverse_system_cases as cs
import inverse_system_ref as isr

pytestmark = pytest.mark.gpu

INVERSE = native.OBJECTIVE_INVERSE_COMPOSITIONAL
H_BAR = 1e-10


def _engine(K, w, h, nl=1, frames=2, depth_range=None, max_iter=None, lam=None, min_grad=None):
    eng = odometry.AlignmentEngine()
    eng.set_config(native.make_config(num_levels=nl, max_iter=max_iter if max_iter else [1] * nl,
                                      min_grad=min_grad if min_grad else [0.0] * nl, lam=lam))
    eng.set_objective(INVERSE)
    eng.set_intrinsic_matrix(K)
    if depth_range is not None:
        eng.set_depth_range(*depth_range)
    eng.reserve_frames(frames, w, h)
    return eng


def _pair_engine(p, nl=1, **kw):
    h, w = p["gray0"].shape
    eng = _engine(p["K"], w, h, nl, **kw)
    eng.upload_frame(0, p["gray0"], p["depth0"])
    eng.upload_frame(1, p["gray1"], p["depth1"])
    return eng


def _set_planes(eng, planes):
    """One level plane by plane: frame 0 the source's four planes, frame 1 the target's intensity (and zero gradient
    planes, which no row reads: writing them gives the frame its target role on the level)."""
    i0, d0, gx0, gy0, i1 = planes
    eng.set_level_planes(0, 0, intensity=i0, depth=d0, grad_x=gx0, grad_y=gy0)
    eng.set_level_planes(1, 0, intensity=i1, grad_x=np.zeros_like(i1), grad_y=np.zeros_like(i1))


def _planes(eng, level, src=0, tgt=1):
    """What the device holds on `level`: (i0, d0, gx0, gy0, i1)."""
    i0, d0, gx0, gy0 = eng.get_level_planes(src, level)
    i1, _, _, _ = eng.get_level_planes(tgt, level)
    return i0, d0, gx0, gy0, i1


def _bytes(structs):
    return [bytes(memoryview(r)) for r in structs]


def _evaluate(eng, states, level=0, src=0, tgt=1):
    states = np.atleast_2d(np.asarray(states, dtype=np.float64))
    n = len(states)
    return eng.evaluate_inverse_pairs([src] * n, [tgt] * n, states, level)


def _hold(part, rec, planes, level, K, states, depth_range=(0.3, 5.0)):
    """Every record of `rec` against the checker; prints the part's worst distances over bar."""
    worst = (0.0, 0.0)
    for k, st in enumerate(np.atleast_2d(states)):
        ref = isr.system(planes, level, K, st, *depth_range)
        try:
            dh, dg = isr.check_record(rec, k, ref)
        except AssertionError as err:
            raise AssertionError(f"{part}, state {k}: {err}") from err
        worst = (max(worst[0], dh), max(worst[1], dg))
    print(f"{part}: worst dH / bar {worst[0]:.3g}, dg / bar {worst[1]:.3g}")
    return worst


# ---- tile geometries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", cs.GEOMETRIES, ids=["%dx%d" % s for s in cs.GEOMETRIES])
def test_tile_geometries(w, h):
    p = cs.geometry_pair(w, h)
    states = cs.three_states(p)
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        rec = _evaluate(eng, states)
    _hold(f"geometry {w}x{h}", rec, planes, 0, p["K"], states)
    if cs.well_posed_size(w, h):
        assert np.all(rec["rows"] >= 6) and not rec["flags"].any()


def test_one_vga_level():
    p = cs.vga_pair()
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        rec = _evaluate(eng, p["motion"])
    _hold("640x480", rec, planes, 0, p["K"], p["motion"])
    assert rec["rows"][0] > 250000 and rec["flags"][0] == 0


# ---- exact positions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,shift,depth_range", cs.EXACT_CASES,
                         ids=[f"{w}x{h}_{s:+.2f}_{r[0]}_{r[1]}" for w, h, s, r in cs.EXACT_CASES])
def test_exact_positions(w, h, shift, depth_range):
    K, planes, state = ie.exact_problem(w, h, shift, depth_range)
    expected = ie.exact_rows(planes[1], shift)
    with _engine(K, w, h, depth_range=depth_range) as eng:
        _set_planes(eng, planes)
        held = _planes(eng, 0)
        rec = _evaluate(eng, state)
    ref = isr.system(held, 0, K, state, *depth_range)
    assert ref[3] == expected and rec["rows"][0] == expected
    _hold(f"exact {w}x{h} {shift:+.2f} {depth_range}", rec, held, 0, K, state, depth_range)


# ---- intrinsics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,shift", cs.K_CASES, ids=[f"{w}x{h}_{s[0]:+.2f}" for w, h, s in cs.K_CASES])
def test_fy_differs_from_fx_and_the_principal_point_is_off_the_grid(w, h, shift):
    p, K = ie.intrinsics_problem(w, h, shift)
    with _engine(K, w, h) as eng:
        eng.upload_frame(0, p["gray0"], p["depth0"])
        eng.upload_frame(1, p["gray1"], p["depth1"])
        planes = _planes(eng, 0)
        rec = _evaluate(eng, ie.K_INIT)
    _hold(f"intrinsics {w}x{h} {shift}", rec, planes, 0, K, ie.K_INIT)
    H = isr.system(planes, 0, K, ie.K_INIT)[0]
    with ie.row_focal_mutant("fy_fx"):
        Hm = isr.system(planes, 0, K, ie.K_INIT)[0]
    assert np.abs(Hm - H).max() > 1e6 * H_BAR * np.abs(H).max()          # the case tells the two rows apart
    assert np.abs(rec["information"][0] - Hm).max() > 1e6 * H_BAR * np.abs(H).max()


# ---- levels 1 and 2 ------------------------------------------------------------------------------------------------------
def test_levels_1_and_2_of_a_three_level_pool():
    p = cs.levels_pair()
    states = cs.three_states(p)
    with _pair_engine(p, nl=3) as eng:
        for level in (1, 2):
            planes = _planes(eng, level)
            assert planes[0].shape == (cs.LEVELS_H >> level, cs.LEVELS_W >> level)
            rec = _evaluate(eng, states, level)
            _hold(f"level {level}", rec, planes, level, p["K"], states)
            assert not rec["flags"].any()


# ---- large rotations -----------------------------------------------------------------------------------------------------
def test_large_rotations_in_one_call():
    p = ie.angle_pair()
    states = cs.angle_states()
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        rec = _evaluate(eng, states)
    _hold("large rotations", rec, planes, 0, p["K"], states)
    lost = np.flatnonzero(rec["rows"] == 0)
    assert len(lost) >= ie.ANGLE_LOST and np.all(rec["rows"][:3] >= 6)
    for k in lost:
        assert rec["flags"][k] == native.PAIR_RANK_DEFICIENT and rec["cost"][k] == 0.0
        assert not rec["information"][k].any() and not rec["gradient"][k].any()


# ---- the aligner's first step is this system ---------------------------------------------------------------------------
@pytest.mark.parametrize("lam", cs.STEP_LAMS)
def test_the_aligners_first_step_is_this_system(lam):
    worst = 0.0
    for i, p in enumerate(cs.step_pairs()):
        for start in (np.zeros(6), cs.STEP_START):
            with _pair_engine(p, lam=[lam]) as eng:
                s, reps = eng.align_pairs([0], [1], init_states=start[None], want_reports=True)
                assert {l["kind"] for l in eng.last_launches()} == {"inverse"}
                rec = _evaluate(eng, start)
            H, g = rec["information"][0], rec["gradient"][0]
            xi = -lam * np.linalg.solve(H, g)                                  # from the RECORD
            R, t = ir.eigen_rt(start)
            ER, Et = ir.se3_exp(xi)
            expect = ir.state_from_pose(R @ ER, R @ Et + t)
            bar = ir.pose_bar(float(np.linalg.cond(H)), expect)
            err = np.abs(s[0] - expect).max()
            worst = max(worst, err / bar)
            assert err <= bar, (i, start, err, bar)
            gn = float(np.linalg.norm(g))
            assert abs(reps[0].gradient_norm - gn) <= 1e-9 * gn
            assert reps[0].valid_pixels[0] == rec["rows"][0] and list(reps[0].iterations[:1]) == [1]
    print(f"first step lambda {lam}: worst distance / bar {worst:.3g}")


# ---- small systems -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,count,const", cs.ROWS_CASES)
def test_small_systems(layout, count, const):
    K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
    with _engine(K, ie.ROWS_W, ie.ROWS_H) as eng:
        _set_planes(eng, planes)
        held = _planes(eng, 0)
        rec = _evaluate(eng, np.zeros(6))
    _hold(f"{layout} {count} rows, constant source {const}", rec, held, 0, K, np.zeros(6))
    assert rec["rows"][0] == count
    assert rec["flags"][0] == (native.PAIR_RANK_DEFICIENT if count < 6 else 0)
    if const:                                                    # H exactly zero with finite sums
        assert not rec["information"][0].any() and not rec["gradient"][0].any() and np.isfinite(rec["cost"][0])


def test_all_nan_depth():
    p = cs.geometry_pair(75, 53)
    p["depth0"] = np.full_like(p["depth0"], np.nan)
    with _pair_engine(p) as eng:
        rec = _evaluate(eng, p["motion"])
    assert rec["rows"][0] == 0 and rec["cost"][0] == 0.0 and rec["flags"][0] == native.PAIR_RANK_DEFICIENT
    assert not rec["information"][0].any() and not rec["gradient"][0].any()


def test_nan_in_the_source_gradient_and_in_unsampled_target_pixels():
    p = cs.geometry_pair(75, 53)
    st = p["motion"] + cs.NAN_SHIFT
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        clean = eng.evaluate_inverse_pairs([0], [1], st[None], 0, want_structs=True)
        _hold("nan planes, clean", clean, planes, 0, p["K"], st)
        # NaN in 200 pixels of GX0 only: rows and cost finite and the checker's, NONFINITE set
        bad = cs.nan_gx_planes(planes)
        eng.set_level_planes(0, 0, grad_x=bad[2])
        rec = _evaluate(eng, st)
        _hold("nan in GX0", rec, _planes(eng, 0), 0, p["K"], st)
        assert rec["flags"][0] == native.PAIR_NONFINITE and rec["rows"][0] == clean["rows"][0]
        assert rec["cost"][0] == clean["cost"][0] and np.isfinite(rec["information"][0][1, 1])
        eng.set_level_planes(0, 0, grad_x=planes[2])
        # NaN in I1 pixels that no row samples: the bytes of the clean record
        hit = isr.sampled_target_pixels(planes, 0, p["K"], st)
        assert (~hit).sum() > 0
        i1 = planes[4].copy()
        i1[~hit] = np.nan
        eng.set_level_planes(1, 0, intensity=i1)
        again = eng.evaluate_inverse_pairs([0], [1], st[None], 0, want_structs=True)
    assert _bytes(again["structs"]) == _bytes(clean["structs"])


# ---- frame pairs of every order ------------------------------------------------------------------------------------------
def test_frame_pairs_of_every_order():
    seq = cs.four_frames()
    states = cs.four_states()
    src, tgt = [a for a, _ in cs.PAIRS_OF_FOUR], [b for _, b in cs.PAIRS_OF_FOUR]
    with _engine(seq["K"], cs.FOUR_W, cs.FOUR_H, frames=4) as eng:
        eng.upload_frames(0, seq["gray"], seq["depth"])
        rec = eng.evaluate_inverse_pairs(src, tgt, states, 0)
        planes = [_planes(eng, 0, a, b) for a, b in cs.PAIRS_OF_FOUR]
    for k in range(len(src)):
        one = {key: rec[key][k:k + 1] for key in rec}
        _hold(f"frames {cs.PAIRS_OF_FOUR[k]}", one, planes[k], 0, seq["K"], states[k])
    assert not rec["flags"].any()


# ---- bit identity --------------------------------------------------------------------------------------------------------
def test_bit_identical_alone_in_a_batch_and_under_every_setting():
    x, y = cs.geometry_pair(75, 53), ie.long_pair()
    assert y["gray0"].shape == (60, 80)
    y = {k: np.ascontiguousarray(v[:53, :75]) for k, v in y.items() if k != "K" and k != "motion"}
    st = np.asarray(x["motion"])
    with _pair_engine(x, frames=4, max_iter=[3]) as eng:
        eng.upload_frame(2, y["gray0"], y["depth0"])
        eng.upload_frame(3, y["gray1"], y["depth1"])

        def alone():
            return _bytes(eng.evaluate_inverse_pairs([0], [1], st[None], 0, want_structs=True)["structs"])[0]
        first = alone()
        rs = np.random.RandomState(1)
        src, tgt, states = [2] * 64, [3] * 64, rs.uniform(-0.02, 0.02, (64, 6))
        src[37], tgt[37], states[37] = 0, 1, st
        got = _bytes(eng.evaluate_inverse_pairs(src, tgt, states, 0, want_structs=True)["structs"])
        assert got[37] == first and got[36] != first
        # the settings DESIGN.md §20 calls "accepted, no effect"
        for setter, values in ((eng.set_level_fusion, [native.FUSION_OFF, native.FUSION_AUTO]), (eng.set_wide_policy, [1, 0]),
                               (eng.set_latency_forms, [True, False]), (eng.set_batch_invariant, [True, False]),
                               (eng.set_slide_policy, [-1, 0])):
            for v in values:
                setter(v)
                assert alone() == first, (setter.__name__, v)
        eng.enqueue_align([0, 2] * 32, [1, 3] * 32)                 # an enqueue in flight before the call
        assert alone() == first
        eng.fetch_results(64)


def test_bit_identical_across_a_group_boundary():
    """874 pairs of 640x480: one more than a group (tile sums of at most 64 MB: 300 tiles x 256 B per pair).  Pairs 0, 872
    and 873 -- the first and the last of the first group and the only one of the second -- have their own frames and state."""
    from phovo_amd import synthetic
    seq = synthetic.make_sequence(33, 3, 640, 480, holes=0.02)
    n = cs.GROUP_PAIRS + 1
    assert n == 874
    src, tgt, states = np.zeros(n, dtype=int), np.ones(n, dtype=int), np.tile(cs.BOUNDARY_STATE, (n, 1))
    for q, (a, b, x) in cs.BOUNDARY_OWN.items():
        src[q], tgt[q], states[q] = a, b, x
    with _engine(seq["K"], 640, 480, frames=3) as eng:
        eng.upload_frames(0, seq["gray"], seq["depth"])

        def alone(a, b, x):
            r = eng.evaluate_inverse_pairs([a], [b], x[None], 0, want_structs=True)
            assert r["rows"][0] > 100000 and r["flags"][0] == 0
            return _bytes(r["structs"])[0]
        one = alone(0, 1, cs.BOUNDARY_STATE)
        singles = {q: alone(*cs.BOUNDARY_OWN[q]) for q in cs.BOUNDARY_OWN}
        got = _bytes(eng.evaluate_inverse_pairs(src, tgt, states, 0, want_structs=True)["structs"])
    assert len({one, *singles.values()}) == 4
    for q in range(n):
        assert got[q] == singles.get(q, one), q


# ---- no interference -----------------------------------------------------------------------------------------------------
def test_no_interference_with_alignments():
    seq = cs.four_frames()
    with _engine(seq["K"], cs.FOUR_W, cs.FOUR_H, frames=4, max_iter=[3]) as eng:
        eng.upload_frames(0, seq["gray"], seq["depth"])
        src, tgt = [0, 1, 2], [1, 2, 3]
        a0, r0 = eng.align_pairs(src, tgt, want_reports=True)
        eng.enqueue_align(src, tgt)
        ticket = eng.last_ticket()
        mid = eng.evaluate_inverse_pairs(src, tgt, a0, 0)
        a1 = eng.fetch(ticket, 3)
        np.testing.assert_array_equal(a0, a1)
        a2, r2 = eng.fetch_results(3, want_reports=True)
        np.testing.assert_array_equal(a0, a2)
        assert _bytes(r0) == _bytes(r2)
        after = eng.evaluate_inverse_pairs(src, tgt, a0, 0)
        np.testing.assert_array_equal(mid["information"], after["information"])
        assert mid["information"].shape == (3, 6, 6) and not mid["flags"].any()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _raw(eng, n, src, tgt, states, level, out):
    return eng._lib.phovo_engine_evaluate_inverse_pairs(eng._h, n, src, tgt, states, level, out)


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except native.PhovoError as err:
        return err.status
    return 0


def test_refusals():
    p = cs.geometry_pair(75, 53)
    s, t = (C.c_int * 1)(0), (C.c_int * 1)(1)
    st = (C.c_double * 6)()
    out = (native.PairSystem * 1)()
    with _pair_engine(p, nl=2) as eng:
        assert _raw(eng, 1, s, t, st, 1, out) == native.OK and out[0].rows > 500
        assert _raw(eng, 0, None, None, None, 1, None) == native.OK
        for args in ((None, t, st, 1, out), (s, None, st, 1, out), (s, t, None, 1, out), (s, t, st, 1, None)):
            assert _raw(eng, 1, *args) == native.E_INVALID_ARGUMENT
        assert _raw(eng, -1, s, t, st, 1, out) == native.E_INVALID_ARGUMENT
        assert _raw(eng, 1, s, t, st, 2, out) == native.E_INVALID_ARGUMENT
        assert _raw(eng, 1, s, t, st, -1, out) == native.E_INVALID_ARGUMENT
        bad = (C.c_int * 1)(2)
        assert _raw(eng, 1, bad, t, st, 1, out) == native.E_INVALID_ARGUMENT
        assert _raw(eng, 1, s, bad, st, 1, out) == native.E_INVALID_ARGUMENT
        # the four older calls stay refused under this objective
        zero6, zero8 = np.zeros((1, 6)), np.zeros((1, 8))
        assert _status(eng.evaluate_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_sampled_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_sampled_pairs, [0], [1], zero8, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_objective_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_geometric_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert b"phovo_engine_evaluate_inverse_pairs" in native.lib().phovo_last_error()
        # every other objective
        for objective in (native.OBJECTIVE_PHOTOMETRIC, native.OBJECTIVE_PHOTOMETRIC_AFFINE,
                          native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC):
            eng.set_objective(objective)
            assert _raw(eng, 1, s, t, st, 1, out) == native.E_UNSUPPORTED
        eng.set_objective(INVERSE)
        assert _raw(eng, 1, s, t, st, 1, out) == native.OK
    for objective in (native.OBJECTIVE_BIOBJECTIVE, native.OBJECTIVE_TRUST_REGION):
        with odometry.AlignmentEngine() as eng:
            eng.set_config(native.make_config(num_levels=2, max_iter=[2, 2], min_grad=[0.0, 0.0]))
            eng.set_objective(objective)
            assert _status(eng.evaluate_inverse_pairs, [0], [1], np.zeros((1, 6)), 0) == native.E_UNSUPPORTED
    with _engine(p["K"], 75, 53) as eng:                         # roles: the source's gradient planes are read
        eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
        eng.upload_frame(1, p["gray1"], p["depth1"])
        assert _status(eng.evaluate_inverse_pairs, [0], [1], np.zeros((1, 6)), 0) == native.E_NOT_READY
        assert b"gradient" in native.lib().phovo_last_error()
        assert _status(eng.evaluate_inverse_pairs, [1], [1], np.zeros((1, 6)), 0) == native.OK
        eng.upload_frame(0, p["gray0"], p["depth0"])
        assert _status(eng.evaluate_inverse_pairs, [0], [1], np.zeros((1, 6)), 0) == native.OK


# ---- the class surface ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter,finest", [([3, 4], 0), ([0, 4], 1)])
def test_class_surface_matches_engine(max_iter, finest):
    p = cs.levels_pair()
    cfg = native.make_config(num_levels=2, max_iter=max_iter, min_grad=[0.0] * 2)
    with odometry.CPhotoconsistencyOdometryInverse() as od:
        od.SetConfiguration(cfg)
        od.SetIntrinsicMatrix(p["K"])
        od.SetSourceFrame(p["gray0"], p["depth0"])
        od.SetTargetFrame(p["gray1"], p["depth1"])
        with pytest.raises(native.PhovoError) as ex:
            od.GetInverseSystem()
        assert ex.value.status == native.E_NOT_READY
        od.Optimize()
        ps = od.GetInverseSystem()
        state = od.GetOptimalStateVector()
        with odometry.AlignmentEngine() as eng:
            eng.set_config(cfg)
            eng.set_objective(INVERSE)
            eng.set_intrinsic_matrix(p["K"])
            eng.reserve_frames(2, cs.LEVELS_W, cs.LEVELS_H)
            eng.upload_frame(0, p["gray0"], p["depth0"])
            eng.upload_frame(1, p["gray1"], p["depth1"])
            ref = eng.evaluate_inverse_pairs([0], [1], state[None], finest, want_structs=True)["structs"][0]
        assert ps.rows > 1000 and ps.flags == 0
        assert bytes(memoryview(ps)) == bytes(memoryview(ref))
        od.SetSourceFrame(p["gray0"], p["depth0"])
        with pytest.raises(native.PhovoError) as ex:
            od.GetInverseSystem()
        assert ex.value.status == native.E_NOT_READY
    with odometry.CPhotoconsistencyOdometryAffine() as od:       # any other objective
        od.SetConfiguration(cfg)
        ps = native.PairSystem()
        assert od._lib.phovo_odometry_get_inverse_system(od._h, C.byref(ps)) == native.E_UNSUPPORTED
