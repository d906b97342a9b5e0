"""The fixtures of tests/inverse_prior_edges.py without a device: each is held to the preconditions
tests/test_gpu_inverse_prior_edges.py relies on -- the checker (tests/inverse_prior_ref.py) against the closed form of the
record, cond(H'), the threshold, bin and delta margins, the angle keep-outs -- and to telling the mutants of the rule it is
there to tell."""
import numpy as np
import pytest

import inverse_edges as ie
import inverse_prior_cases as cases
import inverse_prior_edges as pe
import inverse_prior_ref as pr
import inverse_ref as ir
import inverse_robust_cases as rcases
import inverse_robust_ref as rr

ROBUST = pytest.mark.parametrize("robust", [False, True], ids=pe.OBJECTIVE_NAMES)


def _holds(ref, what, robust):
    assert np.all(np.isfinite(ref["state"])), what
    assert ie.flat(ref), (what, ref["cond"])
    assert ref["margin"] > cases.MARGIN_FLOOR, (what, ref["margin"])
    assert ie.clear_of_the_cuts(ref["state"]), (what, ref["state"])
    assert ref["max_angle"] < cases.MAX_PRIOR_ANGLE, (what, ref["max_angle"])
    if robust:
        assert ref["bin_margin"] >= rcases.BIN_MARGIN_FLOOR, (what, ref["bin_margin"])
        assert ref["delta_margin"] >= rcases.DELTA_MARGIN_FLOOR, (what, ref["delta_margin"])


def _plain(robust):
    return rr.optimize if robust else ir.optimize


# ---- A1 ----------------------------------------------------------------------------------------------------------------------
def test_record_cases_meet_the_closed_form_and_both_sides_of_the_switch():
    """The checker against error = (1 - lambda)^n e_0, the state of T_p Exp(error) and (1 - lambda)^2n e_0^T Lambda e_0 from
    mpmath: within RECORD_CHECKER_WORST absolute on pose and error (measured 1.02e-15, at 3.0 rad), the cost to 8 eps
    relative (measured 1.2e-15).  The recorded angle falls on both sides of Log's series switch and reaches 2.906 rad; every
    state keeps clear of atan2's cuts."""
    p = cases.constant_source_pair()
    pyr = pe.cpu_pyramid(p, 1)
    assert not pyr[0][2].any() and not pyr[0][3].any()
    Lam = pe.record_lambda()
    assert np.linalg.cond(Lam) <= 20
    all_cases = pe.record_cases()
    assert len(all_cases) == 18 == sum(len(pe.record_group(lam, n)) for lam, n in pe.RECORD_STEPS)
    worst, recorded = 0.0, []
    for angle, lam, n, prior, error, cost, state in all_cases:
        prior, error, state = np.array(prior), np.array(error), np.array(state)
        ref = pr.optimize(pyr, p["K"], cases.cfg([n], lam=[lam]), prior, Lam, init_pose=cases.LOG_INIT)
        assert ref["flags"] == 0 and ref["iterations"] == [n] and ref["valid_pixels"][0] >= 6
        d = max(np.abs(ref["state"] - state).max(), np.abs(ref["error"] - error).max())
        worst = max(worst, d)
        assert abs(ref["prior_cost"] - cost) <= 8 * pe.EPS * cost, (angle, lam, n)
        assert ie.clear_of_the_cuts(state), (angle, lam, n, state)
        om = float(np.linalg.norm(error[3:]))
        assert abs(om - (1.0 - lam) ** n * angle) <= 1e-12 * max(1.0, angle / 1e-3)
        recorded.append(om)
    print(f"the checker's worst distance from the closed form: {worst:.3e}")
    assert worst <= pe.RECORD_CHECKER_WORST
    th2 = np.array(recorded) ** 2
    assert np.any(th2 < pr.LOG_SERIES_BELOW) and np.any((th2 > pr.LOG_SERIES_BELOW) & (th2 < 1.1e-8))
    assert min(abs(v - 9.9e-5) for v in recorded) < 1e-12 and min(abs(v - 1.01e-4) for v in recorded) < 1e-12
    assert 2.9 < max(recorded) < cases.MAX_PRIOR_ANGLE
    # the tight bar sits far under the flat one
    flat, eflat, tight, etight = pe.record_bars(np.ones(6), np.ones(6))
    assert tight < 1e-3 * flat and etight < 1e-3 * eflat


def test_record_cases_tell_a_stale_error_and_a_constant_d():
    """What the closed form is there to tell: e taken at the pose BEFORE the last step is e / (1 - lambda), far beyond the
    tight bar at every angle; D held at 1 / 12 moves nu by |D - 1 / 12| |W^2 t| -- beyond the flat error bar from 0.3 rad
    recorded up."""
    for angle, lam, n, prior, error, cost, state in pe.record_cases():
        error = np.array(error)
        flat, eflat, tight, etight = pe.record_bars(np.array(state), error)
        stale = error / (1.0 - lam)
        assert np.abs(stale - error).max() > 1e3 * etight, (angle, lam, n)
        th = float(np.linalg.norm(error[3:]))
        if th >= 0.29:
            D = (1.0 - 0.5 * th / np.tan(0.5 * th)) / (th * th)
            om = error[3:]
            # nu = V^-1 t with V^-1 = I - W / 2 + D W^2: first order in the change of D
            W = ir.hat(om)
            shift = np.abs((D - 1.0 / 12.0) * (W @ W @ np.array(error[:3]))).max()
            assert shift > 10 * eflat, (angle, lam, n, shift)


# ---- A2 ----------------------------------------------------------------------------------------------------------------------
@ROBUST
def test_zero_scale_fixtures(robust):
    p = pe.levels_pair()
    pyr = pe.cpu_pyramid(p, pe.LEVELS_NL)
    costs = []
    for scales in pe.SCALE_LISTS:
        ref = pr.optimize(pyr, p["K"], cases.cfg([5, 5]), cases.PRIOR_STATE, pe.LEVELS_LAMBDA, scales, robust=robust)
        _holds(ref, scales, robust)
        bar = ir.pose_bar(ref["cond"], ref["state"])
        assert np.abs(ref["error"]).max() > 1e3 * 4 * bar         # the record is away from zero: compared in value
        costs.append(ref["prior_cost"])
        ones = pr.optimize(pyr, p["K"], cases.cfg([5, 5]), cases.PRIOR_STATE, pe.LEVELS_LAMBDA, robust=robust)
        assert np.abs(ones["state"] - ref["state"]).max() > 1e3 * bar
    assert abs(costs[0] - costs[1]) > 0.1 * max(costs)


# ---- A3 ----------------------------------------------------------------------------------------------------------------------
@ROBUST
def test_skipped_level_fixtures(robust):
    p = pe.levels_pair()
    pyr = pe.cpu_pyramid(p, pe.LEVELS_NL)
    refs = []
    for mi in pe.SKIP_MAX_ITERS:
        ref = pr.optimize(pyr, p["K"], cases.cfg(mi), cases.PRIOR_STATE, pe.LEVELS_LAMBDA, robust=robust, init_pose=pe.SKIP_INIT)
        assert ref["iterations"] == [m if m > 0 else 1 for m in mi] and ref["flags"] == 0
        assert [v > 0 for v in ref["valid_pixels"]] == [m > 0 for m in mi]
        if any(mi):
            _holds(ref, mi, robust)
        refs.append(ref)
    # the surviving record is the executed level's: the two single-level calls differ, the all-skipped call has none
    assert np.abs(refs[0]["error"] - refs[1]["error"]).max() > 1e-4
    assert refs[2]["state"].tobytes() == pe.SKIP_INIT.tobytes()
    assert not refs[2]["error"].any() and refs[2]["prior_cost"] == 0.0 and refs[2]["gradient_norm"] == 0.0
    assert pe.SKIP_INIT.all()


# ---- A4 ----------------------------------------------------------------------------------------------------------------------
@ROBUST
@pytest.mark.parametrize("k", pe.NONFINITE_ZEROED)
def test_nonfinite_exit_fixtures(k, robust):
    """Lambda_k is positive semidefinite (what the host accepts) and exactly singular; with a constant source H' = Lambda_k:
    the checker leaves the level after ONE iteration of NONFINITE_MAX_ITER with a NaN state.  (i) NONFINITE alone, (ii) with
    RANK_DEFICIENT and no row, (iii) the finer level after a NaN level has no row either."""
    Lam = pe.lambda_zeroed(k)
    assert np.array_equal(Lam, Lam.T) and not Lam[k].any() and np.all(np.diag(Lam) >= 0)
    eig = np.linalg.eigvalsh(Lam)
    assert eig[0] > -1e-12 * eig[-1] and np.linalg.matrix_rank(Lam) == 5
    cfg1, cfg2 = cases.cfg([pe.NONFINITE_MAX_ITER]), cases.cfg([pe.NONFINITE_MAX_ITER] * 2)
    p = cases.constant_source_pair()
    ref = pr.optimize(pe.cpu_pyramid(p, 1), p["K"], cfg1, cases.PRIOR_STATE, Lam, init_pose=cases.LOG_INIT, robust=robust)
    assert np.all(np.isnan(ref["state"])) and ref["flags"] == ir.PAIR_NONFINITE and ref["iterations"] == [1]
    assert ref["valid_pixels"][0] >= 6 and not np.any(np.isfinite(ref["error"]))
    if robust:                                                   # (delta and the outlier count are compared on the device)
        assert ref["bin_margin"] >= rcases.BIN_MARGIN_FLOOR and ref["delta_margin"] >= rcases.DELTA_MARGIN_FLOOR
    q = pe.nan_depth_pair()
    ref = pr.optimize(pe.cpu_pyramid(q, 1), q["K"], cfg1, cases.PRIOR_STATE, Lam, init_pose=cases.LOG_INIT, robust=robust)
    assert np.all(np.isnan(ref["state"])) and ref["flags"] == (ir.PAIR_NONFINITE | ir.PAIR_RANK_DEFICIENT) == 5
    assert ref["iterations"] == [1] and ref["valid_pixels"] == [0]
    ref = pr.optimize(pe.cpu_pyramid(p, 2), p["K"], cfg2, cases.PRIOR_STATE, Lam, init_pose=cases.LOG_INIT, robust=robust)
    assert np.all(np.isnan(ref["state"])) and ref["flags"] == 5 and ref["iterations"] == [1, 1]
    assert ref["valid_pixels"][0] == 0 and ref["valid_pixels"][1] >= 6
    if robust:
        assert ref["bin_margin"] >= rcases.BIN_MARGIN_FLOOR and ref["delta_margin"] >= rcases.DELTA_MARGIN_FLOOR
    # the healthy neighbour of (iv)
    h = pe.levels_pair()
    ref = pr.optimize(pe.cpu_pyramid(h, 1), h["K"], cfg1, cases.PRIOR_STATE, pe.HEALTHY_LAMBDA, robust=robust)
    _holds(ref, "healthy", robust)
    assert ref["flags"] == 0 and ref["iterations"] == [pe.NONFINITE_MAX_ITER]


@ROBUST
@pytest.mark.parametrize("kind", pe.SEMI_KINDS)
def test_semidefinite_fixtures_are_carried_by_the_data(kind, robust):
    p = pe.levels_pair()
    pyr = pe.cpu_pyramid(p, 1)
    Lam = pe.semidefinite_lambda(kind, pe.SEMI_WEIGHT_FRACTION * pe.finest_h00(pyr, p["K"]))
    assert np.linalg.matrix_rank(Lam) == 3
    ref = pr.optimize(pyr, p["K"], cases.cfg([pe.SEMI_ITER]), cases.PRIOR_STATE, Lam, robust=robust)
    _holds(ref, kind, robust)
    assert ref["cond"] <= 1e5 and ref["flags"] == 0
    plain = _plain(robust)(pyr, p["K"], cases.cfg([pe.SEMI_ITER]))
    assert np.abs(plain["state"] - ref["state"]).max() > 1e3 * ir.pose_bar(ref["cond"], ref["state"])


# ---- A5 ----------------------------------------------------------------------------------------------------------------------
def test_triangle_fixtures():
    c = cases.parity_problem(pe.TRIANGLE_PARITY)
    junk = pe.garbage_lower(c["Lambda"])
    assert np.all(np.isfinite(junk)) and np.array_equal(np.triu(junk), np.triu(c["Lambda"]))
    lower = np.tril_indices(6, -1)
    assert np.abs(junk[lower] - c["Lambda"][lower]).min() > 0 and junk[lower].min() < 0
    assert np.array_equal(pr.symmetric_from_upper(junk), c["Lambda"])
    low = pe.lower_only()
    assert np.count_nonzero(low) == 1 and low[4, 1] != 0 and not pr.symmetric_from_upper(low).any()
    # a reader of the lower triangle, or of all 36 entries, would see another matrix
    assert np.abs(pr.symmetric_from_upper(junk.T) - c["Lambda"]).max() > 1.0


# ---- A6 ----------------------------------------------------------------------------------------------------------------------
@ROBUST
def test_termination_norm_fixture_tells_the_data_norm(robust):
    """Measured: the real rule ends after 7 of 12 iterations under both objectives (||g'|| 0.503 -> 0.261 under objective 5,
    0.630 -> 0.385 under objective 6, threshold 0.45); ||g|| never comes under 0.93, so the mutant runs all 12."""
    p = pe.norm_pair()
    pyr = pe.cpu_pyramid(p, 1)
    cfg = cases.cfg(pe.NORM_MAX_ITER, pe.NORM_MIN_GRAD, lam=pe.NORM_LAM)
    ref = pr.optimize(pyr, p["K"], cfg, cases.PRIOR_STATE, pe.NORM_LAMBDA, robust=robust)
    alt = pr.optimize(pyr, p["K"], cfg, cases.PRIOR_STATE, pe.NORM_LAMBDA, robust=robust, mutant="data_norm")
    print(f"real {ref['iterations']} |g'| {ref['gradient_norm']:.4f} margin {ref['margin']:.3e}; "
          f"mutant {alt['iterations']} |g| {alt['gradient_norm']:.4f} margin {alt['margin']:.3e}")
    _holds(ref, "norm", robust)
    assert alt["margin"] > cases.MARGIN_FLOOR
    assert 1 < ref["iterations"][0] < pe.NORM_MAX_ITER[0]
    assert alt["iterations"] != ref["iterations"]
    assert abs(alt["gradient_norm"] - ref["gradient_norm"]) > 1e-3 * ref["gradient_norm"]


# ---- A7 ----------------------------------------------------------------------------------------------------------------------
@ROBUST
@pytest.mark.parametrize("angle", pe.LARGE_ANGLES)
def test_large_error_fixtures(angle, robust):
    p = pe.levels_pair()
    pyr = pe.cpu_pyramid(p, 1)
    Lam = cases.lambda_iso(pe.LARGE_WEIGHT_FRACTION * pe.finest_h00(pyr, p["K"]))
    prior = pe.large_prior_state(angle)
    cfg = cases.cfg([pe.LARGE_ITER])
    ref = pr.optimize(pyr, p["K"], cfg, prior, Lam, robust=robust, init_pose=pe.LARGE_INIT)
    _holds(ref, angle, robust)
    assert angle - 0.1 <= ref["max_angle"] < cases.MAX_PRIOR_ANGLE
    assert ref["flags"] == 0 and ref["valid_pixels"][0] > 400                 # H and g are the data's
    assert np.abs(ref["error"][3:]).max() > 0.5 * angle                       # the data decided: e stays large
    alt = pr.optimize(pyr, p["K"], cfg, prior, Lam, robust=robust, init_pose=pe.LARGE_INIT, mutant="left")
    ratio = np.abs(alt["state"] - ref["state"]).max() / ir.pose_bar(ref["cond"], ref["state"])
    print(f"{angle} rad: cond {ref['cond']:.3g}, the left-hand error ends {ratio:.3g} bars away")
    assert ratio > 1e3
