"""The Gaussian pose prior of the inverse-compositional objectives without a device: the checker
(tests/inverse_prior_ref.py) against exact references and closed forms, the pre-checks of every fixture that
tests/test_gpu_inverse_prior.py runs on the device (tests/inverse_prior_cases.py), the surfaces, and the two mutants of
the rule that the fixtures must tell from the real one."""
import ctypes as C
import os

import mpmath
import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, synthetic
from oracle import numpy_twin as twin

import inverse_edges as ie
import inverse_prior_cases as cases
import inverse_prior_ref as pr
import inverse_ref as ir
import inverse_robust_cases as rcases
import inverse_robust_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


# ---- Log ---------------------------------------------------------------------------------------------------------------
def _logm_exact(R, t):
    """The twist of the matrix logarithm of the fp64 (R, t) as given, in 60 digits."""
    mpmath.mp.dps = 60
    M = mpmath.matrix(4, 4)
    for i in range(3):
        for j in range(3):
            M[i, j] = mpmath.mpf(float(R[i, j]))
        M[i, 3] = mpmath.mpf(float(t[i]))
    M[3, 3] = 1
    G = mpmath.logm(M)
    re = lambda v: float(mpmath.re(v))  # noqa: E731
    return np.array([re(G[0, 3]), re(G[1, 3]), re(G[2, 3]),
                     re(G[2, 1] - G[1, 2]) / 2, re(G[0, 2] - G[2, 0]) / 2, re(G[1, 0] - G[0, 1]) / 2])


def _twists(theta):
    for seed in range(8):
        rs = np.random.RandomState(seed)
        axis = rs.normal(size=3)
        axis /= np.linalg.norm(axis)
        yield seed, np.concatenate([rs.uniform(-0.5, 0.5, 3), theta * axis])


@pytest.mark.parametrize("theta", [0.0, 1e-9, 1e-5, 5e-5, 9.9e-5, 1.01e-4, 1e-3, 0.3, 1.0, 2.0, 3.0])
def test_se3_log_against_the_exact_matrix_logarithm(theta):
    """Both sides of the series switch (th^2 = 1e-8 at th = 1e-4) and up to |omega| = 3.  Bar: 4 ulp of the largest entry of
    the exact twist; the worst case measured over these inputs is 2.0 ulp (at 1e-3 and at 1.0) -- se3_exp's test in
    test_inverse_cpu.py measures 3.5 ulp under the same bar of 4."""
    worst = 0.0
    for seed, xi in _twists(theta):
        R, t = ir.se3_exp(xi)
        got, exact = pr.se3_log(R, t), _logm_exact(R, t)
        bar = 4 * np.spacing(np.abs(exact).max())
        err = np.abs(got - exact).max()
        worst = max(worst, err / bar)
        assert err <= bar, (seed, err, bar)
    print(f"theta {theta}: worst error / bar = {worst:.3f}")


@pytest.mark.parametrize("theta", [0.0, 1e-7, 5e-5, 9.9e-5, 1.01e-4, 1e-3, 0.3, 1.0, 2.0, 3.0])
def test_log_undoes_exp(theta):
    """Log(Exp(xi)) = xi.  Exp is good to 4 ulp of its largest entry (at most 1 here) and Log to 4 ulp; Log turns an error
    of R into one of omega with the factor th / sin th, which is below 1.2 up to 1 rad and 1 / sin th = 7.1 at 3 rad.  Bar:
    8 eps x max(1.2, th / sin th) x max(1, |xi|); measured: 6.7e-16 at 3 rad (bar 3.8e-14), 2.2e-16 at 1 rad."""
    amplification = 1.2 if theta <= 1.0 else theta / np.sin(theta)
    worst = 0.0
    for seed, xi in _twists(theta):
        back = pr.se3_log(*ir.se3_exp(xi))
        bar = 8 * EPS * amplification * max(1.0, np.abs(xi).max())
        err = np.abs(back - xi).max()
        worst = max(worst, err / bar)
        assert err <= bar, (seed, err, bar)
    assert (theta * theta < pr.LOG_SERIES_BELOW) == (theta < 1e-4)
    print(f"theta {theta}: worst error / bar = {worst:.3f}")


# ---- the rule ------------------------------------------------------------------------------------------------------------
def _same_record(a, b):
    for key in b:
        va, vb = np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64)
        assert va.tobytes() == vb.tobytes(), (key, a[key], b[key])


@pytest.mark.parametrize("robust", [False, True])
def test_lambda_zero_is_the_checker_without_a_prior_bit_for_bit(robust):
    p = cases.small_pair(1, 24, 20)
    pyr = ie.twin_pyramid(p, 2)
    cfg = cases.cfg([6, 6], [0.6, 0.5], lam=[0.9, 0.8])
    plain = rr.optimize(pyr, p["K"], cfg) if robust else ir.optimize(pyr, p["K"], cfg)
    for Lam, scales in ((np.zeros((6, 6)), None), (cases.lambda_full(1, 100.0), [0.0, 0.0])):
        got = pr.optimize(pyr, p["K"], cfg, cases.PRIOR_STATE, Lam, scales, robust=robust)
        _same_record(got, plain)
        assert got["prior_cost"] == (0.0 if not Lam.any() else got["prior_cost"]) and got["max_angle"] == 0.0
    moved = pr.optimize(pyr, p["K"], cfg, cases.PRIOR_STATE, cases.lambda_full(1, 100.0), robust=robust)
    assert np.abs(moved["state"] - plain["state"]).max() > 1e-6


def _constant_planes(w=24, h=20, seed=3):
    rs = np.random.RandomState(seed)
    i0 = np.full((h, w), 0.5)
    return (i0, rs.uniform(1.0, 3.0, (h, w)), np.zeros((h, w)), np.zeros((h, w)), rs.uniform(0, 1, (h, w)))


@pytest.mark.parametrize("Lam", [cases.lambda_iso(1.0), cases.lambda_iso(1e-6), cases.lambda_full(2, 1.0),
                                 cases.lambda_full(3, 1e4)], ids=["I", "1e-6 I", "full", "1e4 full"])
def test_constant_source_lands_on_the_prior_in_one_iteration(Lam):
    """H and g are exactly zero: H' = Lambda, g' = Lambda e, xi = -e and T Exp(-Log(T_p^-1 T)) = T_p, for any positive
    definite Lambda.  Bar: the round trip's (Log, a solve with cond(Lambda) <= 20, Exp, one composition) on angles below
    0.01: 16 eps x max(1, |x|); measured 5.6e-17."""
    K = synthetic.intrinsics(24, 20)
    planes = _constant_planes()
    assert not ir.system(planes, 0, K, np.eye(3), np.zeros(3))[1].any()
    assert np.linalg.cond(Lam) <= 20
    for init in (None, np.array([0.02, 0.01, -0.015, -0.003, 0.006, 0.002])):
        ref = pr.optimize([planes], K, cases.cfg([1]), cases.PRIOR_STATE, Lam, init_pose=init)
        err = np.abs(ref["state"] - cases.PRIOR_STATE).max()
        print(f"distance from the prior {err:.2e}")
        assert ref["flags"] == 0 and ref["iterations"] == [1] and err <= 16 * EPS
        assert np.abs(ref["error"]).max() <= 16 * EPS and ref["prior_cost"] <= (16 * EPS) ** 2 * np.abs(Lam).sum()


def aperture_planes():
    """160x120, every row the same textured row, the target the source rolled by one column, depth 2 m: nothing constrains
    y, and z and the rotations only through x's coupling."""
    w, h = 160, 120
    x = np.arange(w)
    row = 0.5 + 0.25 * np.sin(x / 5.0) + 0.15 * np.sin(x / 2.3 + 1.0) + 0.05 * np.random.RandomState(0).uniform(-1, 1, w)
    i0 = np.tile(row, (h, 1))
    gx0, gy0 = twin.scharr(i0, ie.GRAD_SCALE)
    return synthetic.intrinsics(w, h), (i0, np.full((h, w), 2.0), gx0, gy0, np.roll(i0, 1, axis=1))


def test_aperture_pair_moves_along_x_and_stays_at_the_prior_elsewhere():
    """Measured: the smallest eigenvalue of H is -2.2e-10 (the largest 7e6), the plain checker's solve is singular; with
    Lambda = 1e-3 I and a zero prior, 10 iterations end at x = 0.015213 (one pixel at 2 m is 2 / fx = 0.015238; 30 iterations:
    0.0152381), |z| = 1.5e-6, |pitch| = 4.5e-6, everything else below 1e-12.  Asserted: x within 1 % of the pixel, the
    other five below 1e-5 (twice the largest measured)."""
    K, planes = aperture_planes()
    assert not planes[3].any()
    eig = np.linalg.eigvalsh(ir.system(planes, 0, K, np.eye(3), np.zeros(3))[1])
    print(f"eigenvalues of H: {eig[0]:.2e} ... {eig[-1]:.2e}")
    assert abs(eig[0]) < 1e-15 * eig[-1] * 1e2
    plain = ir.optimize([planes], K, cases.cfg([10]))
    assert plain["flags"] & ir.PAIR_NONFINITE and np.all(np.isnan(plain["state"])) and plain["cond"] == np.inf
    ref = pr.optimize([planes], K, cases.cfg([10]), np.zeros(6), cases.lambda_iso(1e-3))
    print(ref["state"])
    pixel = 2.0 / K[0, 0]
    assert ref["flags"] == 0 and abs(ref["state"][0] - pixel) <= 0.01 * pixel
    assert np.abs(ref["state"][1:]).max() <= 1e-5


def test_textured_pair_under_a_weak_and_a_rigid_prior():
    """synthetic.make_pair(1, 160, 120), 3 levels x 10 iterations, zero prior.  Lambda = I leaves the result where it is
    without a prior (1.26e-4 from the generator's motion against 1.22e-4: both under the 1e-3 the accuracy tests ask);
    Lambda = 1e9 I holds the pose at the prior: ||g|| <= 2e3 against 1e9 moves it 1.7e-6, asserted below 1e-5."""
    p = synthetic.make_pair(1, 160, 120)
    pyr = ie.twin_pyramid(p, 3)
    cfg = cases.cfg([10, 10, 10])
    none = ir.optimize(pyr, p["K"], cfg)
    weak = pr.optimize(pyr, p["K"], cfg, np.zeros(6), cases.lambda_iso(1.0))
    rigid = pr.optimize(pyr, p["K"], cfg, np.zeros(6), cases.lambda_iso(1e9))
    d_none, d_weak = np.abs(none["state"] - p["motion"]).max(), np.abs(weak["state"] - p["motion"]).max()
    d_rigid = np.abs(rigid["state"]).max()
    print(f"from the truth: none {d_none:.3e}, I {d_weak:.3e}; 1e9 I stays {d_rigid:.3e} from the prior")
    assert d_none <= 1e-3 and d_weak <= 1e-3
    assert 0.0 < d_rigid <= 1e-5
    assert np.abs(p["motion"]).max() > 1e-3                       # the truth is a thousand times further away


@pytest.mark.parametrize("robust", [False, True])
def test_a_zero_level_scale_is_no_prior_on_that_level(robust):
    """level_scale = [0, 1]: level 1 runs with the prior, level 0 without -- bit for bit the two levels run apart, the
    second by the checker that knows no prior."""
    p = cases.small_pair(1, 24, 20)
    pyr = ie.twin_pyramid(p, 2)
    Lam = cases.lambda_full(4, 100.0)
    both = pr.optimize(pyr, p["K"], cases.cfg([5, 5]), cases.PRIOR_STATE, Lam, [0.0, 1.0], robust=robust)
    coarse = pr.optimize(pyr, p["K"], cases.cfg([0, 5]), cases.PRIOR_STATE, Lam, [1.0, 1.0], robust=robust)
    plain = rr.optimize if robust else ir.optimize
    fine = plain(pyr, p["K"], cases.cfg([5, 0]), init_pose=coarse["state"])
    assert both["state"].tobytes() == fine["state"].tobytes()
    assert both["gradient_norm"] == fine["gradient_norm"]
    everywhere = pr.optimize(pyr, p["K"], cases.cfg([5, 5]), cases.PRIOR_STATE, Lam, [1.0, 1.0], robust=robust)
    assert np.abs(everywhere["state"] - both["state"]).max() > 1e-6


# ---- every GPU fixture's pre-check ---------------------------------------------------------------------------------------
def _holds(ref, what, robust):
    assert np.all(np.isfinite(ref["state"])), what
    assert ie.flat(ref), (what, ref["cond"])                      # cond(H') <= 1e5: the flat 1e-9 bar
    assert ref["margin"] > cases.MARGIN_FLOOR, (what, ref["margin"])
    assert ie.clear_of_the_cuts(ref["state"]), (what, ref["state"])
    assert ref["max_angle"] < cases.MAX_PRIOR_ANGLE, (what, ref["max_angle"])
    if robust:
        assert ref["bin_margin"] >= rcases.BIN_MARGIN_FLOOR, (what, ref["bin_margin"])
        assert ref["delta_margin"] >= rcases.DELTA_MARGIN_FLOOR, (what, ref["delta_margin"])


def _cpu_pyramid(p, nl):
    h, w = p["gray0"].shape
    return ie.twin_pyramid(p, nl) if (w % 2 ** (nl - 1) == 0 and h % 2 ** (nl - 1) == 0 and nl > 1) else ie.oracle_pyramid(p, nl)


@pytest.mark.parametrize("robust", [False, True], ids=["objective5", "objective6"])
@pytest.mark.parametrize("name", list(cases.PARITY))
def test_parity_fixtures_hold_the_flat_bar_and_tell_the_mutants(name, robust):
    """The pre-check, and the mutants: the checker with e taken on the left, Log(T T_p^-1), or with s_L Lambda e subtracted,
    ends more than 1000 pose bars away on the fixtures meant to catch it -- the sign on every parity fixture, the side on
    those whose name is in SIDE_CATCHERS (a left and a right error differ in second order, |omega| |nu|)."""
    c = cases.parity_problem(name)
    pyr = _cpu_pyramid(c["p"], c["nl"])
    cfg = cases.cfg(c["mi"], c["mg"], lam=c["lam"])
    ref = pr.optimize(pyr, c["K"], cfg, c["prior"], c["Lambda"], c["scales"], robust=robust)
    _holds(ref, name, robust)
    print(f"{name}: iterations {ref['iterations']} cond {ref['cond']:.2e} margin {ref['margin']:.2e} |e| {np.abs(ref['error']).max():.2e}")
    assert ref["flags"] == 0
    if any(c["mg"]):
        assert all(1 < it < m for it, m in zip(ref["iterations"], c["mi"])), ref["iterations"]
    else:
        assert ref["iterations"] == c["mi"]
    plain = (rr.optimize if robust else ir.optimize)(pyr, c["K"], cfg)
    bar = ir.pose_bar(ref["cond"], ref["state"])
    assert np.abs(plain["state"] - ref["state"]).max() > 1e3 * bar          # the prior moves the result
    for mutant in ("minus", "left"):
        alt = pr.optimize(pyr, c["K"], cfg, c["prior"], c["Lambda"], c["scales"], robust=robust, mutant=mutant)
        ratio = np.abs(alt["state"] - ref["state"]).max() / bar
        print(f"  mutant {mutant}: {ratio:.3g} bars away")
        if mutant == "minus" or name in SIDE_CATCHERS:
            assert ratio > 1e3, (name, mutant, ratio)
    ones = pr.optimize(pyr, c["K"], cfg, c["prior"], c["Lambda"], None, robust=robust)     # s_L dropped
    if any(s != 1.0 for s in c["scales"]):
        assert np.abs(ones["state"] - ref["state"]).max() > 1e3 * bar


SIDE_CATCHERS = ("24x20 full", "75x53 full", "80x60 iso", "160x120 three levels")


def test_log_regime_fixtures():
    """The prior poses of the device's Log test: every regime of the series switch and of the sin / cos branches is met, the
    states keep clear of atan2's cuts, and the left-hand mutant misses the prior by more than 1000 bars from 0.3 rad up."""
    expected = {5e-5: True, 9.9e-5: True, 1.01e-4: False, 0.3: False, 0.783: False, 0.80: False, 1.2: False, 2.0: False,
                3.0: False}
    assert tuple(expected) == cases.LOG_ANGLES
    K = synthetic.intrinsics(cases.LOG_W, cases.LOG_H)
    planes = _constant_planes(cases.LOG_W, cases.LOG_H)
    for angle in cases.LOG_ANGLES:
        prior = cases.log_prior_state(angle)
        assert ie.clear_of_the_cuts(prior), (angle, prior)
        e = pr.prior_error(*ir.eigen_rt(cases.LOG_INIT), *ir.eigen_rt(prior))
        assert (float(e[3:] @ e[3:]) < pr.LOG_SERIES_BELOW) == expected[angle]
        assert abs(np.linalg.norm(e[3:]) - angle) <= 1e-12 * max(1.0, angle / 1e-3) and angle <= cases.MAX_PRIOR_ANGLE
        ref = pr.optimize([planes], K, cases.cfg([1]), prior, cases.lambda_full(5, 10.0), init_pose=cases.LOG_INIT)
        bar = 1e-9 * max(1.0, np.abs(prior).max())
        assert ref["flags"] == 0 and np.abs(ref["state"] - prior).max() <= bar
        alt = pr.optimize([planes], K, cases.cfg([1]), prior, cases.lambda_full(5, 10.0), init_pose=cases.LOG_INIT,
                          mutant="left")
        if angle >= 0.3:
            assert np.abs(alt["state"] - prior).max() > 1e3 * bar, angle


@pytest.mark.parametrize("robust", [False, True], ids=["objective5", "objective6"])
@pytest.mark.parametrize("layout,count,const", cases.ROWS_CASES)
def test_row_count_fixtures_are_finite_under_the_prior(layout, count, const, robust):
    """5, 6 and 7 rows, and the constant source's exactly zero H: with a positive definite Lambda every pose is finite;
    RANK_DEFICIENT follows the row count alone, NONFINITE is never set."""
    K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
    plain = ir.optimize([planes], K, cases.cfg([ie.ROWS_ITER]))
    ref = pr.optimize([planes], K, cases.cfg([ie.ROWS_ITER]), cases.PRIOR_STATE, cases.ROWS_LAMBDA, robust=robust)
    if robust:
        assert ref["bin_margin"] >= rcases.BIN_MARGIN_FLOOR and ref["delta_margin"] >= rcases.DELTA_MARGIN_FLOOR
    print(f"{layout} {count} {const}: cond {ref['cond']:.2e}, plain flags {plain['flags']}")
    assert ref["valid_pixels"] == [count] and ref["iterations"] == [ie.ROWS_ITER]
    assert ref["flags"] == (ir.PAIR_RANK_DEFICIENT if count < 6 else 0)
    assert np.all(np.isfinite(ref["state"])) and ie.clear_of_the_cuts(ref["state"]) and ref["cond"] < 1e7
    if count < 6:
        assert plain["flags"] & ir.PAIR_RANK_DEFICIENT           # (without a prior: a NaN pose, or one made of rounding noise)
    if const:
        assert plain["flags"] & ir.PAIR_NONFINITE
    if const:
        assert np.abs(ref["state"] - cases.PRIOR_STATE).max() <= 1e-12


def test_work_queue_fixtures():
    """Every (pair, prior pose, Lambda) combination of the list holds the flat bar, or is the lost pair D: NaN under every
    prior (no row: the pose constants are never written from a finite H' alone -- Lambda = 0 -- or finite otherwise)."""
    pairs = ie.work_queue_pairs()
    states, lambdas, pick_s, pick_l = cases.work_queue_priors(1541)
    assert set(pick_s.tolist()) == set(range(cases.WQ_PRIORS)) and set(pick_l.tolist()) == set(range(cases.WQ_LAMBDAS))
    assert not lambdas[0].any() and all(np.all(np.linalg.eigvalsh(m) > 0) for m in lambdas[1:])
    cfg = cases.cfg(cases.WQ_MAX_ITER, cases.WQ_MIN_GRAD)
    for i, p in enumerate(pairs):
        pyr = ie.twin_pyramid(p, ie.WQ_LEVELS)
        for a in range(cases.WQ_PRIORS):
            for b in range(cases.WQ_LAMBDAS):
                ref = pr.optimize(pyr, p["K"], cfg, states[a], lambdas[b])
                if i == ie.WQ_D and b == 0:
                    assert np.all(np.isnan(ref["state"]))
                    continue
                assert np.all(np.isfinite(ref["state"])), (i, a, b)
                assert ie.flat(ref) and ref["margin"] > cases.MARGIN_FLOOR, (i, a, b, ref["cond"], ref["margin"])
                if i == ie.WQ_D:
                    assert ref["flags"] == ir.PAIR_RANK_DEFICIENT and ref["valid_pixels"] == [0, 0]


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_the_surface_is_there():
    assert native.LAUNCH_KINDS[12] == "inverse_prior" and native.LAUNCH_KINDS[13] == "inverse_robust_prior"
    L = native.lib()
    for name in ("phovo_prior_options_default", "phovo_engine_set_prior_options", "phovo_engine_get_prior_options",
                 "phovo_engine_enqueue_align_prior", "phovo_engine_fetch_prior_reports", "phovo_odometry_set_pose_prior",
                 "phovo_odometry_clear_pose_prior", "phovo_odometry_get_prior_report", "phovo_odometry_set_prior_options",
                 "phovo_odometry_get_prior_options", "phovo_prior_report_format"):
        assert hasattr(L, name), name
    for cls in (odometry.CPhotoconsistencyOdometryInverse, odometry.CPhotoconsistencyOdometryRobust):
        for method in ("SetPosePrior", "ClearPosePrior", "GetPriorReport", "SetPriorOptions", "GetPriorOptions"):
            assert hasattr(cls, method), (cls, method)
    assert not hasattr(odometry.CPhotoconsistencyOdometryAnalytic, "SetPosePrior")
    for method in ("set_prior_options", "get_prior_options", "fetch_prior_reports"):
        assert hasattr(odometry.AlignmentEngine, method)
    header = open(os.path.join(ROOT, "include", "phovo_hip.h")).read()
    assert "PHOVO_LAUNCH_INVERSE_PRIOR = 12" in header and "PHOVO_LAUNCH_INVERSE_ROBUST_PRIOR = 13" in header
    assert "g + s_L Lambda e = 0" in header and "D = 1 / 12 + th^2 / 720 + th^4 / 30240" in header
    assert "int phovo_engine_fetch_prior_reports(phovo_engine *e, int n_pairs, phovo_prior_report *reports);" in header
    assert C.sizeof(native.PriorReport) == 56 == odometry.PRIOR_REPORT_DTYPE.itemsize
    assert C.sizeof(native.PriorOptions) == 8 * native.MAX_LEVELS
    opt = native.make_prior_options()
    assert list(opt.level_scale) == [1.0] * native.MAX_LEVELS
    assert list(native.make_prior_options([0.5, 2.0]).level_scale[:3]) == [0.5, 2.0, 1.0]


def test_arguments_are_checked_without_a_device():
    L = native.lib()
    assert L.phovo_prior_options_default(None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_set_prior_options(None, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_get_prior_options(None, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_fetch_prior_reports(None, 0, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_enqueue_align_prior(None, 0, None, None, None, None, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_set_pose_prior(None, None, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_clear_pose_prior(None) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_get_prior_report(None, None) == native.E_INVALID_ARGUMENT
    eng = object.__new__(odometry.AlignmentEngine)              # the wrapper's own checks come before any native call
    for kw in (dict(prior_states=np.zeros((1, 6))), dict(information=np.zeros((1, 6, 6)))):
        with pytest.raises(ValueError):
            eng.enqueue_align([0], [1], **kw)
    with pytest.raises(ValueError):
        eng.enqueue_align([0], [1], prior_states=np.zeros((1, 5)), information=np.zeros((1, 6, 6)))
    po = object.__new__(odometry.CPhotoconsistencyOdometryInverse)
    for state, info in ((np.zeros(5), np.eye(6)), (np.zeros(6), np.eye(5))):
        with pytest.raises(ValueError):
            po.SetPosePrior(state, info)


def test_the_format_line_round_trips():
    rep = native.PriorReport()
    values = [0.1, -2.5e-7, 1.0 / 3.0, -0.0123456789012345678, 5e-5, 3.0]
    for i, v in enumerate(values):
        rep.error[i] = v
    rep.prior_cost = 1.0 / 7.0
    line = native.format_prior_report(12.5, rep)
    fields = line.split(" ")
    assert len(fields) == 8 and "\n" not in line
    assert [float(f) for f in fields] == [12.5, 1.0 / 7.0] + values
    L = native.lib()
    buf = C.create_string_buffer(8)
    assert L.phovo_prior_report_format(12.5, C.byref(rep), buf, 8) == native.E_INVALID_ARGUMENT
    assert L.phovo_prior_report_format(12.5, None, buf, 8) == native.E_INVALID_ARGUMENT


# ---- the app's flag, as far as it goes without a device ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vo_app():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])
    return os.path.join(ROOT, "apps", "bin", "PhotoconsistencyVisualOdometry")


@pytest.mark.parametrize("extra,needle", [
    (["--batch", "--method", "inverse", "--prior-weight", "1,1"], "cannot be combined with --batch"),
    (["--prior-weight", "1,1"], "--prior-weight needs --method inverse or --method robust"),
    (["--method", "geometric", "--prior-weight", "1,1"], "--prior-weight needs --method inverse or --method robust"),
    (["--method", "robust", "--prior-weight", "1;1"], "--prior-weight needs <wt>,<wr>"),
    (["--method", "robust", "--prior-weight", "-1,1"], "--prior-weight needs <wt>,<wr>"),
    (["--method", "robust", "--prior-weight", "1,inf"], "--prior-weight needs <wt>,<wr>"),
])
def test_the_app_refuses_the_flag_where_it_cannot_apply(vo_app, tmp_path, extra, needle):
    import subprocess
    r = subprocess.run([vo_app, "cfg.yml", str(tmp_path), str(tmp_path / "t.txt")] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and needle in r.stderr
    usage = subprocess.run([vo_app], capture_output=True, text=True, timeout=60)
    assert usage.returncode != 0 and usage.stdout.rstrip().endswith("[--prior-weight <wt>,<wr>]")
    assert "affine|geometric]" in usage.stdout and "[--robust-system <file>]" in usage.stdout
