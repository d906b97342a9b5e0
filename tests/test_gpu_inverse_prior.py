"""GPU tests of the Gaussian pose prior of the two inverse-compositional objectives (phovo_engine_enqueue_align_prior,
gn_inverse_prior_kernel.hip) against its CPU checker (tests/inverse_prior_ref.py) fed the planes exactly as
the device holds them.  Iterations, rows, flags (and, under objective 6, outliers) exact; the pose to inverse_ref.pose_bar
(the flat 1e-9 x max(1, |x|) on every fixture: tests/test_inverse_prior_cpu.py holds cond(H') below 1e5 without a device);
gradient_norm, the norm of g' = g + s_L Lambda e, to 1e-9 relative.  Every enqueue asserts its launch kind."""
import ctypes as C

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

import inverse_edges as ie
import inverse_prior_cases as cases
import inverse_prior_ref as pr
import inverse_ref as ir
import inverse_robust_cases as rcases

pytestmark = pytest.mark.gpu

INVERSE, ROBUST = native.OBJECTIVE_INVERSE_COMPOSITIONAL, native.OBJECTIVE_INVERSE_ROBUST
OBJECTIVES = [INVERSE, ROBUST]
IDS = ["objective5", "objective6"]
KIND = {INVERSE: ("inverse", "inverse_prior", 1696), ROBUST: ("inverse_robust", "inverse_robust_prior", 18112)}
BOTH = ir.PAIR_RANK_DEFICIENT | ir.PAIR_NONFINITE


def _engine(objective, K, w, h, frames, mi, mg=None, lam=None, scales=None):
    nl = len(mi)
    eng = odometry.AlignmentEngine()
    eng.set_config(native.make_config(num_levels=nl, max_iter=mi, min_grad=mg if mg else [0.0] * nl, lam=lam))
    eng.set_objective(objective)
    if scales is not None:
        eng.set_prior_options(native.make_prior_options(scales))
    eng.set_intrinsic_matrix(K)
    eng.reserve_frames(frames, w, h)
    return eng


def _upload(eng, pairs):
    """Pair i: source frame 2 i, target frame 2 i + 1."""
    for i, p in enumerate(pairs):
        eng.upload_frame(2 * i, p["gray0"], p["depth0"])
        eng.upload_frame(2 * i + 1, p["gray1"], p["depth1"])


def _device_pyramid(eng, src, tgt, nl, mi):
    pyr = []
    for l in range(nl):
        if mi[l] <= 0:
            pyr.append(None)
            continue
        i0, d0, gx0, gy0 = eng.get_level_planes(src, l)
        i1, _, _, _ = eng.get_level_planes(tgt, l)
        pyr.append((i0, d0, gx0, gy0, i1))
    return pyr


def _kinds(eng, objective, prior=True):
    launches = eng.last_launches()
    assert launches and {l["kind"] for l in launches} == {KIND[objective][1 if prior else 0]}
    assert {l["threads"] for l in launches} == {256}
    if prior:
        assert {l["lds_bytes"] for l in launches} == {KIND[objective][2]}
    return launches


def _align(eng, objective, src, tgt, priors, infos, inits=None):
    """One enqueue with a prior -> (states, reports, prior reports, robust reports or None)."""
    n = eng.enqueue_align(src, tgt, init_states=inits, prior_states=priors, information=infos)
    _kinds(eng, objective)
    s, reps = eng.fetch_results(n, want_reports=True)
    rob = eng.fetch_robust_reports(n) if objective == ROBUST else None
    return s, reps, eng.fetch_prior_reports(n), rob


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _record(s, rep, prep, rob, nl):
    """Everything a pair reports, for bit-for-bit comparison."""
    out = [_bits(s), list(rep.iterations[:nl]), list(rep.valid_pixels[:nl]), int(rep.flags), _bits([rep.gradient_norm])]
    if prep is not None:
        out += [_bits(prep["error"]), _bits([prep["prior_cost"]])]
    if rob is not None:
        out += [_bits(rob["delta"][:nl]), list(rob["outliers"][:nl])]
    return out


def _ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b), 2.0 ** -1000))


def _compare(s, rep, prep, rob, ref, Lam, nl, margins=True):
    print(f"device it {list(rep.iterations[:nl])} valid {list(rep.valid_pixels[:nl])} flags {rep.flags} state {s} |g'| "
          f"{rep.gradient_norm}; checker {ref['iterations']} {ref['valid_pixels']} {ref['flags']} {ref['state']} "
          f"{ref['gradient_norm']} cond {ref['cond']:.3e} margin {ref['margin']:.3e}")
    if margins:
        assert ref["margin"] > cases.MARGIN_FLOOR, "fixture too close to its gradient threshold"
        assert ref["max_angle"] < cases.MAX_PRIOR_ANGLE
        if rob is not None:
            assert ref["bin_margin"] >= rcases.BIN_MARGIN_FLOOR and ref["delta_margin"] >= rcases.DELTA_MARGIN_FLOOR
    assert list(rep.iterations[:nl]) == ref["iterations"]
    assert list(rep.valid_pixels[:nl]) == ref["valid_pixels"]
    assert int(rep.flags) == ref["flags"]
    if rob is not None:
        assert list(rob["outliers"][:nl]) == ref["outliers"]
        for l in range(nl):
            assert _ulps(float(rob["delta"][l]), ref["delta"][l]) <= 4, (l, rob["delta"][l], ref["delta"][l])
    if not np.all(np.isfinite(ref["state"])):
        assert not np.any(np.isfinite(s[~np.isfinite(ref["state"])]))
        return 0.0
    bar = ir.pose_bar(ref["cond"], ref["state"])
    err = np.abs(s - ref["state"]).max()
    print(f"max |device - checker| = {err:.3e}, bar {bar:.1e}")
    assert err <= bar
    assert abs(rep.gradient_norm - ref["gradient_norm"]) <= 1e-9 * max(1.0, ref["gradient_norm"])
    # e = Log(T_p^-1 T): its entries are combinations of the six pose errors with coefficients below 1 (|t| < 1, angles
    # below 1 rad: Log's Jacobian stays below 1.2) -- 4 pose bars; e^T Lambda e follows with the factor 2 |Lambda e|_1
    ebar = 4 * bar
    assert np.abs(prep["error"] - ref["error"]).max() <= ebar
    cbar = 2 * np.abs(pr.symmetric_from_upper(Lam) @ ref["error"]).sum() * ebar + 1e-9 * abs(ref["prior_cost"])
    assert abs(prep["prior_cost"] - ref["prior_cost"]) <= cbar, (prep["prior_cost"], ref["prior_cost"], cbar)
    return err / bar


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("name", list(cases.PARITY))
def test_parity_with_the_checker(name, objective):
    c = cases.parity_problem(name)
    p, nl = c["p"], c["nl"]
    h, w = p["gray0"].shape
    with _engine(objective, c["K"], w, h, 2, c["mi"], c["mg"], c["lam"], c["scales"]) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, nl, c["mi"])
        s, reps, preps, rob = _align(eng, objective, [0], [1], [c["prior"]], [c["Lambda"]])
        assert all(l["workgroups"] == 1 for l in eng.last_launches()) and len(eng.last_launches()) == nl
    ref = pr.optimize(pyr, c["K"], cases.cfg(c["mi"], c["mg"], lam=c["lam"]), c["prior"], c["Lambda"], c["scales"],
                      robust=objective == ROBUST)
    ratio = _compare(s[0], reps[0], preps[0], None if rob is None else rob[0], ref, c["Lambda"], nl)
    assert ie.flat(ref) and ref["flags"] == 0
    if any(c["mg"]):
        assert all(1 < it < m for it, m in zip(ref["iterations"], c["mi"])), ref["iterations"]      # by the thresholds
    print(f"{name}: distance / bar {ratio:.3g}")


# ---- 2. Lambda = 0, and s_L = 0: the bits of the call without a prior ------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
def test_zero_information_and_zero_scale_are_the_call_without_a_prior_bit_for_bit(objective):
    make_x, make_y, nl, mi, mg = rcases.IDENTITY
    x, y = make_x(), make_y()
    src, tgt = [0, 2, 0], [1, 3, 1]
    priors = np.tile(cases.PRIOR_STATE, (3, 1))
    zero, full = np.zeros((3, 6, 6)), np.stack([cases.lambda_full(7, 4000.0)] * 3)
    with _engine(objective, x["K"], 80, 60, 4, mi, mg) as eng:
        _upload(eng, [x, y])
        s, reps = eng.align_pairs(src, tgt, want_reports=True)
        _kinds(eng, objective, prior=False)
        rob = eng.fetch_robust_reports(3) if objective == ROBUST else [None] * 3
        plain = [_record(s[k], reps[k], None, rob[k], nl) for k in range(3)]
        assert plain[0] == plain[2] != plain[1]
        s, reps, preps, rob = _align(eng, objective, src, tgt, priors, zero)
        rob = [None] * 3 if rob is None else rob
        assert [_record(s[k], reps[k], None, rob[k], nl) for k in range(3)] == plain
        assert not preps["prior_cost"].any() and np.all(np.isfinite(preps["error"])) and preps["error"].any()
        moved, _, mp, _ = _align(eng, objective, src, tgt, priors, full)
        assert _bits(moved) != _bits(s) and np.all(mp["prior_cost"] > 0)
        eng.set_prior_options(native.make_prior_options([0.0] * nl))
        s, reps, preps, rob = _align(eng, objective, src, tgt, priors, full)
        rob = [None] * 3 if rob is None else rob
        assert [_record(s[k], reps[k], None, rob[k], nl) for k in range(3)] == plain
        assert np.all(preps["prior_cost"] > 0)                     # e^T Lambda e is reported without s_L


# ---- 3. Log's regimes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("rows", ["every_pixel", "no_row"])
def test_log_regimes_land_on_the_prior(rows, objective):
    """A constant source: H and g are exactly zero, so with lambda = 1 one iteration is T Exp(-Log(T_p^-1 T)) = T_p.  The
    prior sits 5e-5 ... 3.0 rad about a skew axis from the start (both sides of Log's series switch, th / 2 on both sides
    of pi / 4, atan2 far from its first octant).  RANK_DEFICIENT as the rows say, NONFINITE never."""
    p = cases.constant_source_pair()
    if rows == "no_row":
        p["depth0"] = np.full_like(p["depth0"], np.nan)
    Lam = cases.lambda_full(5, 10.0)
    n = len(cases.LOG_ANGLES)
    priors = np.stack([cases.log_prior_state(a) for a in cases.LOG_ANGLES])
    with _engine(objective, p["K"], cases.LOG_W, cases.LOG_H, 2, [1]) as eng:
        _upload(eng, [p])
        i0, d0, gx0, gy0 = eng.get_level_planes(0, 0)
        assert not gx0.any() and not gy0.any()
        s, reps, preps, _ = _align(eng, objective, [0] * n, [1] * n, priors, np.stack([Lam] * n), np.tile(cases.LOG_INIT, (n, 1)))
    for k, angle in enumerate(cases.LOG_ANGLES):
        bar = 1e-9 * max(1.0, np.abs(priors[k]).max())
        err = np.abs(s[k] - priors[k]).max()
        print(f"{angle} rad: |device - prior| = {err:.2e}, |e| = {np.abs(preps['error'][k]).max():.2e}")
        assert (reps[k].valid_pixels[0] == 0) if rows == "no_row" else (reps[k].valid_pixels[0] >= 6)
        assert list(reps[k].iterations[:1]) == [1]
        assert int(reps[k].flags) == (ir.PAIR_RANK_DEFICIENT if rows == "no_row" else 0)
        assert err <= bar
        assert np.abs(preps["error"][k]).max() <= 4 * bar and abs(preps["prior_cost"][k]) <= 1e-12


# ---- 4. five, six and seven rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("layout,count,const", cases.ROWS_CASES)
def test_row_count_systems_are_finite_and_the_checkers(layout, count, const, objective):
    K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
    mi = [ie.ROWS_ITER]
    with _engine(objective, K, ie.ROWS_W, ie.ROWS_H, 2, mi) as eng:
        i0, d0, gx0, gy0, i1 = planes
        eng.set_level_planes(0, 0, intensity=i0, depth=d0, grad_x=gx0, grad_y=gy0)
        eng.set_level_planes(1, 0, intensity=i1)
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        s, reps, preps, rob = _align(eng, objective, [0], [1], [cases.PRIOR_STATE], [cases.ROWS_LAMBDA])
    ref = pr.optimize(pyr, K, cases.cfg(mi), cases.PRIOR_STATE, cases.ROWS_LAMBDA, robust=objective == ROBUST)
    assert ref["valid_pixels"] == [count] and ref["flags"] == (ir.PAIR_RANK_DEFICIENT if count < 6 else 0)
    assert np.all(np.isfinite(s[0]))
    _compare(s[0], reps[0], preps[0], None if rob is None else rob[0], ref, cases.ROWS_LAMBDA, 1)


# ---- 5. the work queue -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
def test_work_queue_every_position_keeps_its_own_prior(objective):
    """N = 3 G + 5 pairs (G: the persistent grid), every position with a prior pose and an information matrix of its own
    (among them Lambda = 0, and the pair whose source depth is all NaN): every position has the bits of the same pair aligned
    alone under the same prior -- a block that survived from the pair before on a workgroup would break that.  Three
    enqueues in a row take both slots; then two are in flight with DIFFERENT priors on the same pairs, fetched by ticket."""
    nl = ie.WQ_LEVELS
    pairs = ie.work_queue_pairs()
    K = pairs[0]["K"]
    with _engine(objective, K, ie.WQ_W, ie.WQ_H, 8, cases.WQ_MAX_ITER, cases.WQ_MIN_GRAD) as eng:
        _upload(eng, pairs)
        eng.align_pairs([0] * 4096, [1] * 4096)
        G = eng.last_launches()[0]["workgroups"]
        N = 3 * G + 5
        which = ie.work_queue_list(N)
        states, lambdas, ps, pl = cases.work_queue_priors(N)
        combos = sorted({(int(a), int(b), int(c)) for a, b, c in zip(which, ps, pl)})
        assert {a for a, _, _ in combos} == {0, 1, 2, 3} and {c for _, _, c in combos} == set(range(cases.WQ_LAMBDAS))
        alone = {}
        for a, b, c in combos:
            s, reps, preps, rob = _align(eng, objective, [2 * a], [2 * a + 1], [states[b]], [lambdas[c]])
            alone[(a, b, c)] = _record(s[0], reps[0], preps[0], None if rob is None else rob[0], nl)
            assert np.all(np.isnan(s[0])) == (a == ie.WQ_D and c == 0), (a, b, c, s[0])
            if a == ie.WQ_D:
                assert int(reps[0].flags) == (BOTH if c == 0 else ir.PAIR_RANK_DEFICIENT)
        assert len({repr(v) for v in alone.values()}) > len(combos) // 2
        tickets = []
        for run in range(3):
            s, reps, preps, rob = _align(eng, objective, 2 * which, 2 * which + 1, states[ps], lambdas[pl])
            tickets.append(eng.last_ticket())
            launches = eng.last_launches()
            assert len(launches) == nl and all(l["workgroups"] == G < N for l in launches)
            for k in range(N):
                got = _record(s[k], reps[k], preps[k], None if rob is None else rob[k], nl)
                assert got == alone[(int(which[k]), int(ps[k]), int(pl[k]))], (run, k)
        assert {t % 2 for t in tickets} == {0, 1}                 # both slots
        # two enqueues in flight, the second with every position's prior moved on by one
        ps2, pl2 = np.roll(ps, 1), np.roll(pl, 1)
        missing = sorted({(int(a), int(b), int(c)) for a, b, c in zip(which, ps2, pl2)} - set(alone))
        for a, b, c in missing:
            s, reps, preps, rob = _align(eng, objective, [2 * a], [2 * a + 1], [states[b]], [lambdas[c]])
            alone[(a, b, c)] = _record(s[0], reps[0], preps[0], None if rob is None else rob[0], nl)
        eng.enqueue_align(2 * which, 2 * which + 1, prior_states=states[ps], information=lambdas[pl])
        _kinds(eng, objective)
        t1 = eng.last_ticket()
        eng.enqueue_align(2 * which, 2 * which + 1, prior_states=states[ps2], information=lambdas[pl2])
        _kinds(eng, objective)
        t2 = eng.last_ticket()
        # (the prior and the robust records speak of the LAST enqueue only: the second's are compared in full, the first's
        # pose, counts, flags and gradient norm)
        s, reps = eng.fetch(t1, N, want_reports=True)
        for k in range(N):
            assert _record(s[k], reps[k], None, None, nl) == alone[(int(which[k]), int(ps[k]), int(pl[k]))][:5], (t1, k)
        s, reps = eng.fetch(t2, N, want_reports=True)
        preps = eng.fetch_prior_reports(N)
        rob = eng.fetch_robust_reports(N) if objective == ROBUST else None
        for k in range(N):
            got = _record(s[k], reps[k], preps[k], None if rob is None else rob[k], nl)
            assert got == alone[(int(which[k]), int(ps2[k]), int(pl2[k]))], (t2, k)


# ---- 6. the records' fetch rules ---------------------------------------------------------------------------------------------
def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except native.PhovoError as err:
        return err.status
    return 0


def test_prior_reports_follow_the_fetch_rules():
    p = cases.small_pair(1, 24, 20)
    with _engine(INVERSE, p["K"], 24, 20, 2, [3]) as eng:
        _upload(eng, [p])
        assert _status(eng.fetch_prior_reports, 1) == native.E_NOT_READY
        eng.align_pairs([0], [1])
        assert _status(eng.fetch_prior_reports, 1) == native.E_UNSUPPORTED          # the last enqueue carried no prior
        s, reps, preps, _ = _align(eng, INVERSE, [0, 0], [1, 1], [cases.PRIOR_STATE] * 2, [cases.lambda_iso(100.0)] * 2)
        assert _status(eng.fetch_prior_reports, 1) == native.E_INVALID_ARGUMENT     # n_pairs differs from the enqueue's
        again = eng.fetch_prior_reports(2)
        assert again.tobytes() == preps.tobytes() and _bits(preps["error"][0]) == _bits(preps["error"][1])
        assert eng.enqueue_align([], [], prior_states=np.zeros((0, 6)), information=np.zeros((0, 36))) == 0
        assert len(eng.fetch_prior_reports(0)) == 0
        eng.align_pairs([0], [1])
        assert _status(eng.fetch_prior_reports, 1) == native.E_UNSUPPORTED


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    p = cases.small_pair(1, 24, 20)
    good_s, good_l = np.array([cases.PRIOR_STATE]), np.array([cases.lambda_iso(10.0)])
    for objective in (native.OBJECTIVE_PHOTOMETRIC, native.OBJECTIVE_BIOBJECTIVE, native.OBJECTIVE_TRUST_REGION,
                      native.OBJECTIVE_PHOTOMETRIC_AFFINE, native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC):
        with odometry.AlignmentEngine() as eng:
            eng.set_objective(objective)
            assert _status(eng.enqueue_align, [0], [1], prior_states=good_s, information=good_l) == native.E_UNSUPPORTED
            # the options are kept under every objective
            eng.set_prior_options(native.make_prior_options([0.5, 2.0]))
            assert list(eng.get_prior_options().level_scale[:3]) == [0.5, 2.0, 1.0]
    with _engine(INVERSE, p["K"], 24, 20, 2, [3]) as eng:
        _upload(eng, [p])
        first = eng.align_pairs([0], [1])
        ticket = eng.last_ticket()
        for bad in (np.nan, np.inf, -np.inf):
            s, l = good_s.copy(), good_l.copy()
            s[0, 4] = bad
            assert _status(eng.enqueue_align, [0], [1], prior_states=s, information=good_l) == native.E_INVALID_ARGUMENT
            l[0, 1, 2] = bad                                     # (an entry of the upper triangle)
            assert _status(eng.enqueue_align, [0], [1], prior_states=good_s, information=l) == native.E_INVALID_ARGUMENT
        l = good_l.copy()
        l[0, 3, 3] = -1e-300
        assert _status(eng.enqueue_align, [0], [1], prior_states=good_s, information=l) == native.E_INVALID_ARGUMENT
        lib, ip = native.lib(), C.POINTER(C.c_int)
        one = np.zeros(1, dtype=np.int32)
        assert lib.phovo_engine_enqueue_align_prior(eng._h, 1, one.ctypes.data_as(ip), one.ctypes.data_as(ip), None, None,
                                                    None) == native.E_INVALID_ARGUMENT
        # a refused enqueue leaves the engine as it was
        assert eng.last_ticket() == ticket and _bits(eng.fetch(ticket, 1)) == _bits(first)
        for bad in ([-1.0], [np.nan], [np.inf], [1.0, -0.5]):
            assert _status(eng.set_prior_options, native.make_prior_options(bad)) == native.E_INVALID_ARGUMENT
        assert list(eng.get_prior_options().level_scale) == [1.0] * native.MAX_LEVELS
        eng.set_prior_options(native.make_prior_options([0.0]))                       # 0 is allowed
        l = good_l.copy()
        l[0, 2, 2] = 0.0                                         # and so is a zero on the diagonal
        assert _status(eng.enqueue_align, [0], [1], prior_states=good_s, information=l) == 0
        _kinds(eng, INVERSE)


# ---- 8. the class surface in Python ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
def test_class_surface_carries_the_prior(objective):
    c = cases.parity_problem("24x20 two levels by threshold")
    p, nl = c["p"], c["nl"]
    ncfg = native.make_config(num_levels=nl, max_iter=c["mi"], min_grad=c["mg"], lam=c["lam"])
    with _engine(objective, c["K"], 24, 20, 2, c["mi"], c["mg"], c["lam"], c["scales"]) as eng:
        _upload(eng, [p])
        s, reps, preps, _ = _align(eng, objective, [0], [1], [c["prior"]], [c["Lambda"]])
        plain = eng.align_pairs([0], [1])
    cls = odometry.CPhotoconsistencyOdometryInverse if objective == INVERSE else odometry.CPhotoconsistencyOdometryRobust
    with cls(0) as po:
        po.SetConfiguration(ncfg)
        po.SetIntrinsicMatrix(c["K"])
        po.SetPriorOptions(native.make_prior_options(c["scales"]))
        assert list(po.GetPriorOptions().level_scale[:nl]) == c["scales"]
        po.SetSourceFrame(p["gray0"], p["depth0"])
        po.SetTargetFrame(p["gray1"], p["depth1"])
        po.SetPosePrior(c["prior"], c["Lambda"])
        po.Optimize()
        assert _bits(po.GetOptimalStateVector()) == _bits(s[0])
        rep = po.GetPriorReport()
        assert _bits(list(rep.error)) == _bits(preps["error"][0]) and rep.prior_cost == preps["prior_cost"][0]
        line = native.format_prior_report(1.5, rep).split(" ")
        assert [float(v) for v in line[2:]] == list(rep.error) and float(line[1]) == rep.prior_cost
        po.ClearPosePrior()
        po.SetInitialStateVector(np.zeros(6))                     # (Optimize() starts from the current state vector)
        po.Optimize()
        assert _bits(po.GetOptimalStateVector()) == _bits(plain[0])
        with pytest.raises(native.PhovoError) as err:
            po.GetPriorReport()
        assert err.value.status == native.E_UNSUPPORTED
        for state, info in ((np.full(6, np.nan), np.eye(6)), (np.zeros(6), -np.eye(6))):
            with pytest.raises(native.PhovoError) as err:
                po.SetPosePrior(state, info)
            assert err.value.status == native.E_INVALID_ARGUMENT
    # any other objective refuses Optimize() while a prior is set (the C ABI: the Python classes of the others have no setter)
    with odometry.CPhotoconsistencyOdometryAnalytic(0) as pa:
        pa.SetConfiguration(ncfg)
        pa.SetIntrinsicMatrix(c["K"])
        pa.SetSourceFrame(p["gray0"], p["depth0"])
        pa.SetTargetFrame(p["gray1"], p["depth1"])
        dp = C.POINTER(C.c_double)
        st, info = np.array(c["prior"]), np.ascontiguousarray(c["Lambda"]).reshape(-1)
        native.check(pa._lib.phovo_odometry_set_pose_prior(pa._h, st.ctypes.data_as(dp), info.ctypes.data_as(dp)), "prior")
        assert pa._lib.phovo_odometry_optimize(pa._h) == native.E_UNSUPPORTED
        native.check(pa._lib.phovo_odometry_clear_pose_prior(pa._h), "clear")
        pa.Optimize()
