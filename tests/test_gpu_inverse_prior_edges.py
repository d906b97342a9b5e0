"""GPU tests of the pose prior's record, exits and level edges (gn_inverse_prior_kernel.hip, gn_inverse_prior_device.hpp,
phovo_engine_enqueue_align_prior) on the fixtures of tests/inverse_prior_edges.py, which
tests/test_inverse_prior_edges_cpu.py holds to their preconditions without a device.  Every case runs under both objectives,
asserts its launch kind and LDS size, and feeds the checker (tests/inverse_prior_ref.py) the planes read back from the device;
the bars are test_gpu_inverse_prior._compare's unless a test states its own."""
import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native

import inverse_edges as ie
import inverse_prior_cases as cases
import inverse_prior_edges as pe
import inverse_prior_ref as pr
import inverse_ref as ir
from test_gpu_inverse_prior import (BOTH, IDS, OBJECTIVES, ROBUST, _align, _bits, _compare, _device_pyramid, _engine, _kinds,
                                    _record, _upload)

pytestmark = pytest.mark.gpu


def _plain(eng, objective, src, tgt, nl, inits=None):
    """align_pairs without a prior -> the records of its pairs (no prior record)."""
    s, reps = eng.align_pairs(src, tgt, init_states=inits, want_reports=True)
    _kinds(eng, objective, prior=False)
    rob = eng.fetch_robust_reports(len(src)) if objective == ROBUST else [None] * len(src)
    return s, reps, [_record(s[k], reps[k], None, rob[k], nl) for k in range(len(src))]


def _rob(rob, k):
    return None if rob is None else rob[k]


# ---- A1. the record's Log regimes, by the closed form ----------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("lam,n", pe.RECORD_STEPS, ids=[f"lambda{lam:g}x{n}" for lam, n in pe.RECORD_STEPS])
def test_record_meets_the_closed_form_in_every_log_regime(lam, n, objective):
    """A constant source, H = g = 0 exactly: after n iterations of step length lambda the pose is T_p Exp((1 - lambda)^n e_0),
    so the record is error = (1 - lambda)^n e_0 and prior_cost = (1 - lambda)^2n e_0^T Lambda e_0, with e_0 from a 60-digit
    matrix logarithm -- no checker in between.  The recorded angle lies on both sides of Log's series switch (9.9e-5,
    1.01e-4) and reaches 2.906 rad; a record taken at the pose before the last step would be 1 / (1 - lambda) times too large.
    Hard bar: the flat 1e-9 x max(1, |x|) on the pose and 4 of it on the error.  Tight bar: 256 x the checker's own worst
    distance from the closed form over the same 18 inputs (1.3e-15, tests/test_inverse_prior_edges_cpu.py), floored at
    64 eps x max(1, |x|): 3.3e-13.  The factor stands for the device's sincos / atan2 (a few ulp, tests/test_gpu_device_arith.py),
    a 6 x 6 solve with cond(Lambda) <= 20, Exp, one composition and the second Log."""
    p = cases.constant_source_pair()
    group = pe.record_group(lam, n)
    Lam = pe.record_lambda()
    m = len(group)
    priors = np.array([c[3] for c in group])
    with _engine(objective, p["K"], cases.LOG_W, cases.LOG_H, 2, [n], lam=[lam]) as eng:
        _upload(eng, [p])
        _, _, gx0, gy0 = eng.get_level_planes(0, 0)
        assert not gx0.any() and not gy0.any()
        s, reps, preps, _ = _align(eng, objective, [0] * m, [1] * m, priors, np.stack([Lam] * m), np.tile(cases.LOG_INIT, (m, 1)))
    worst = 0.0
    for k, (angle, _, _, _, error, cost, state) in enumerate(group):
        error, state = np.array(error), np.array(state)
        flat, eflat, tight, etight = pe.record_bars(state, error)
        ds, de = np.abs(s[k] - state).max(), np.abs(preps["error"][k] - error).max()
        dc = abs(preps["prior_cost"][k] - cost)
        le = np.abs(Lam @ error).sum()
        print(f"{angle} rad, lambda {lam:g}, n {n}: |state - closed form| = {ds:.3e}, |error - closed form| = {de:.3e} "
              f"(tight bars {tight:.1e}, {etight:.1e}), prior_cost off by {dc:.3e} of {cost:.3e}")
        worst = max(worst, ds, de)
        assert list(reps[k].iterations[:1]) == [n] and int(reps[k].flags) == 0 and reps[k].valid_pixels[0] >= 6
        assert ds <= flat and de <= eflat and dc <= 2 * le * eflat + 1e-9 * cost
        assert ds <= tight and de <= etight, (angle, ds, de)
        assert dc <= 2 * le * etight + 64 * pe.EPS * cost
    print(f"the device's worst distance from the closed form: {worst:.3e}")


# ---- A2. a zero scale on some levels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
def test_zero_scale_on_one_level_records_what_the_checker_records(objective):
    """level_scale [0, 1] and [1, 0]: the level with scale 0 takes the section without a prior and still leaves the record --
    error and prior_cost are compared in value.  [0, 1] is also, bit for bit, the prior call on level 1 alone followed by
    the call without a prior on level 0 alone."""
    p = pe.levels_pair()
    nl, mi, Lam = pe.LEVELS_NL, [5, 5], pe.LEVELS_LAMBDA
    costs = []
    for scales in pe.SCALE_LISTS:
        with _engine(objective, p["K"], pe.LEVELS_W, pe.LEVELS_H, 2, mi, scales=scales) as eng:
            _upload(eng, [p])
            pyr = _device_pyramid(eng, 0, 1, nl, mi)
            s, reps, preps, rob = _align(eng, objective, [0], [1], [cases.PRIOR_STATE], [Lam])
            assert [l["levels"] for l in eng.last_launches()] == [[1], [0]]
        ref = pr.optimize(pyr, p["K"], cases.cfg(mi), cases.PRIOR_STATE, Lam, scales, robust=objective == ROBUST)
        _compare(s[0], reps[0], preps[0], _rob(rob, 0), ref, Lam, nl)
        assert ie.flat(ref) and ref["flags"] == 0 and np.abs(ref["error"]).max() > 1e-3
        costs.append(float(preps["prior_cost"][0]))
        if scales == [0.0, 1.0]:
            whole = (_bits(s[0]), _bits([reps[0].gradient_norm]))
    assert abs(costs[0] - costs[1]) > 0.1 * max(costs)
    with _engine(objective, p["K"], pe.LEVELS_W, pe.LEVELS_H, 2, [0, 5]) as eng:
        _upload(eng, [p])
        coarse, _, _, _ = _align(eng, objective, [0], [1], [cases.PRIOR_STATE], [Lam])
    with _engine(objective, p["K"], pe.LEVELS_W, pe.LEVELS_H, 2, [5, 0]) as eng:
        _upload(eng, [p])
        fine, freps, _ = _plain(eng, objective, [0], [1], nl, inits=coarse)
    assert (_bits(fine[0]), _bits([freps[0].gradient_norm])) == whole


# ---- A3. skipped levels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("mi", pe.SKIP_MAX_ITERS, ids=[str(m) for m in pe.SKIP_MAX_ITERS])
def test_skipped_levels_under_a_prior(mi, objective):
    """max_iter [0, 5], [5, 0], [0, 0] from a non-zero start: the record that survives is the executed level's; with every
    level skipped nothing is launched (the engine's level loop passes every level by), the state is the start bit for bit
    and the record is all zeros."""
    p = pe.levels_pair()
    nl, Lam = pe.LEVELS_NL, pe.LEVELS_LAMBDA
    with _engine(objective, p["K"], pe.LEVELS_W, pe.LEVELS_H, 2, mi) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, nl, mi)
        n = eng.enqueue_align([0], [1], init_states=[pe.SKIP_INIT], prior_states=[cases.PRIOR_STATE], information=[Lam])
        launches = eng.last_launches()
        if any(mi):
            _kinds(eng, objective)
        assert [l["levels"] for l in launches] == [[l] for l in (1, 0) if mi[l] > 0]
        s, reps = eng.fetch_results(n, want_reports=True)
        preps = eng.fetch_prior_reports(n)
        rob = eng.fetch_robust_reports(n) if objective == ROBUST else None
    ref = pr.optimize(pyr, p["K"], cases.cfg(mi), cases.PRIOR_STATE, Lam, robust=objective == ROBUST, init_pose=pe.SKIP_INIT)
    _compare(s[0], reps[0], preps[0], _rob(rob, 0), ref, Lam, nl)
    assert list(reps[0].iterations[:nl]) == [m if m > 0 else 1 for m in mi]
    if not any(mi):
        assert launches == [] and _bits(s[0]) == _bits(pe.SKIP_INIT) and int(reps[0].flags) == 0
        assert not preps["error"][0].any() and preps["prior_cost"][0] == 0.0 and reps[0].gradient_norm == 0.0
        assert list(reps[0].valid_pixels[:nl]) == [0, 0]
    else:
        assert np.abs(preps["error"][0]).max() > 1e-4


# ---- A4. the serial section's non-finite exit, and semidefinite Lambda ----------------------------------------------------------
def _nonfinite(s, rep, prep, flags):
    assert np.all(np.isnan(s)) and int(rep.flags) == flags
    assert not np.any(np.isfinite(prep["error"])) and not np.isfinite(prep["prior_cost"])


@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("k", pe.NONFINITE_ZEROED)
def test_singular_system_leaves_through_the_nonfinite_exit(k, objective):
    """Lambda_k (lambda_full(5, 10.0) with row and column k zeroed: positive semidefinite, a legal call) on a constant
    source: H' = s Lambda_k is exactly singular.  (i) every depth valid: the state all NaN, NONFINITE alone, ONE iteration of
    the four allowed, a non-finite record; (ii) an all-NaN source depth: NONFINITE | RANK_DEFICIENT, no row; (iii) two
    levels: level 1 ends NaN, level 0 runs from the NaN state and reports what the checker reports."""
    Lam = pe.lambda_zeroed(k)
    robust = objective == ROBUST
    mi = [pe.NONFINITE_MAX_ITER]
    p, q = cases.constant_source_pair(), pe.nan_depth_pair()
    with _engine(objective, p["K"], cases.LOG_W, cases.LOG_H, 4, mi) as eng:
        _upload(eng, [p, q])
        pyrs = [_device_pyramid(eng, 0, 1, 1, mi), _device_pyramid(eng, 2, 3, 1, mi)]
        s, reps, preps, rob = _align(eng, objective, [0, 2], [1, 3], [cases.PRIOR_STATE] * 2, [Lam] * 2, [cases.LOG_INIT] * 2)
    for i, flags in enumerate((ir.PAIR_NONFINITE, BOTH)):
        ref = pr.optimize(pyrs[i], p["K"], cases.cfg(mi), cases.PRIOR_STATE, Lam, robust=robust, init_pose=cases.LOG_INIT)
        assert ref["flags"] == flags and ref["iterations"] == [1] and np.all(np.isnan(ref["state"]))
        _compare(s[i], reps[i], preps[i], _rob(rob, i), ref, Lam, 1, margins=False)
        _nonfinite(s[i], reps[i], preps[i], flags)
        assert list(reps[i].iterations[:1]) == [1] and (reps[i].valid_pixels[0] == 0) == (i == 1)
    mi2 = [pe.NONFINITE_MAX_ITER] * 2
    with _engine(objective, p["K"], cases.LOG_W, cases.LOG_H, 2, mi2) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 2, mi2)
        s, reps, preps, rob = _align(eng, objective, [0], [1], [cases.PRIOR_STATE], [Lam], [cases.LOG_INIT])
        assert [l["levels"] for l in eng.last_launches()] == [[1], [0]]
    ref = pr.optimize(pyr, p["K"], cases.cfg(mi2), cases.PRIOR_STATE, Lam, robust=robust, init_pose=cases.LOG_INIT)
    assert ref["flags"] == BOTH and ref["iterations"] == [1, 1] and ref["valid_pixels"][0] == 0 < ref["valid_pixels"][1]
    _compare(s[0], reps[0], preps[0], _rob(rob, 0), ref, Lam, 2, margins=False)
    _nonfinite(s[0], reps[0], preps[0], BOTH)


@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
def test_a_nan_pair_leaves_nothing_behind_for_the_next_pair_of_its_workgroup(objective):
    """2 G + 3 positions (G: the persistent grid), the singular pair of (i) alternating with a healthy pair under a prior of
    its own: every healthy position has the bits of that pair aligned alone, every singular position those of the singular
    pair alone -- no NaN and no flag crosses through the LDS block or the control words."""
    mi = [pe.NONFINITE_MAX_ITER]
    bad, good = cases.constant_source_pair(), pe.levels_pair()
    Lam_bad, Lam_good = pe.lambda_zeroed(pe.NONFINITE_ZEROED[0]), pe.HEALTHY_LAMBDA
    with _engine(objective, bad["K"], cases.LOG_W, cases.LOG_H, 4, mi) as eng:
        _upload(eng, [bad, good])
        eng.align_pairs([0] * 4096, [1] * 4096)
        G = eng.last_launches()[0]["workgroups"]
        N = 2 * G + 3
        alone = []
        for i, (Lam, init) in enumerate(((Lam_bad, cases.LOG_INIT), (Lam_good, np.zeros(6)))):
            s, reps, preps, rob = _align(eng, objective, [2 * i], [2 * i + 1], [cases.PRIOR_STATE], [Lam], [init])
            alone.append(_record(s[0], reps[0], preps[0], _rob(rob, 0), 1))
            assert np.all(np.isnan(s[0])) == (i == 0) and int(reps[0].flags) == (ir.PAIR_NONFINITE if i == 0 else 0)
        which = np.arange(N) % 2
        infos = np.where(which[:, None, None] == 0, Lam_bad, Lam_good)
        inits = np.where(which[:, None] == 0, cases.LOG_INIT, np.zeros(6))
        s, reps, preps, rob = _align(eng, objective, 2 * which, 2 * which + 1, np.tile(cases.PRIOR_STATE, (N, 1)), infos, inits)
        launches = eng.last_launches()
        assert len(launches) == 1 and launches[0]["workgroups"] == G < N
    for k in range(N):
        assert _record(s[k], reps[k], preps[k], _rob(rob, k), 1) == alone[which[k]], k


@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("kind", pe.SEMI_KINDS)
def test_rotation_only_and_translation_only_priors(kind, objective):
    """A textured pair under Lambda = diag(0, 0, 0, w, w, w), and under diag(w, w, w, 0, 0, 0): the data carries the other
    three directions, the result is finite and the checker's."""
    p = pe.levels_pair()
    mi = [pe.SEMI_ITER]
    with _engine(objective, p["K"], pe.SEMI_W, pe.SEMI_H, 2, mi) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        Lam = pe.semidefinite_lambda(kind, pe.SEMI_WEIGHT_FRACTION * pe.finest_h00(pyr, p["K"]))
        s, reps, preps, rob = _align(eng, objective, [0], [1], [cases.PRIOR_STATE], [Lam])
    ref = pr.optimize(pyr, p["K"], cases.cfg(mi), cases.PRIOR_STATE, Lam, robust=objective == ROBUST)
    assert ie.flat(ref) and ref["flags"] == 0 and np.all(np.isfinite(s[0]))
    _compare(s[0], reps[0], preps[0], _rob(rob, 0), ref, Lam, 1)


# ---- A5. the upper triangle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
def test_only_the_upper_triangle_is_read(objective):
    """A lower triangle of finite garbage changes no bit of anything reported; a Lambda whose only non-zero entry lies below
    the diagonal is no prior: the bits of the call without one, prior_cost 0."""
    c = cases.parity_problem(pe.TRIANGLE_PARITY)
    p, nl = c["p"], c["nl"]
    h, w = p["gray0"].shape
    with _engine(objective, c["K"], w, h, 2, c["mi"], c["mg"], c["lam"], c["scales"]) as eng:
        _upload(eng, [p])
        got = []
        for Lam in (c["Lambda"], pe.garbage_lower(c["Lambda"]), pe.lower_only()):
            s, reps, preps, rob = _align(eng, objective, [0], [1], [c["prior"]], [Lam])
            got.append(_record(s[0], reps[0], preps[0], _rob(rob, 0), nl))
            cost = float(preps["prior_cost"][0])
        _, _, plain = _plain(eng, objective, [0], [1], nl)
    assert got[1] == got[0]
    assert got[2][:5] + got[2][7:] == plain[0] and cost == 0.0 and got[2][:5] != got[0][:5]


# ---- A6. the termination norm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
def test_the_level_ends_on_the_norm_of_the_posterior_gradient(objective):
    """The fixture on which ||g'|| < threshold and ||g|| < threshold end the level after different iteration counts
    (tests/test_inverse_prior_edges_cpu.py): the device's count and gradient_norm are the real rule's."""
    p = pe.norm_pair()
    mi, mg = pe.NORM_MAX_ITER, pe.NORM_MIN_GRAD
    h, w = p["gray0"].shape
    robust = objective == ROBUST
    with _engine(objective, p["K"], w, h, 2, mi, mg, pe.NORM_LAM) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        s, reps, preps, rob = _align(eng, objective, [0], [1], [cases.PRIOR_STATE], [pe.NORM_LAMBDA])
    cfg = cases.cfg(mi, mg, lam=pe.NORM_LAM)
    ref = pr.optimize(pyr, p["K"], cfg, cases.PRIOR_STATE, pe.NORM_LAMBDA, robust=robust)
    alt = pr.optimize(pyr, p["K"], cfg, cases.PRIOR_STATE, pe.NORM_LAMBDA, robust=robust, mutant="data_norm")
    assert alt["iterations"] != ref["iterations"] and alt["margin"] > cases.MARGIN_FLOOR
    _compare(s[0], reps[0], preps[0], _rob(rob, 0), ref, pe.NORM_LAMBDA, 1)
    assert list(reps[0].iterations[:1]) == ref["iterations"] != alt["iterations"]
    assert abs(reps[0].gradient_norm - alt["gradient_norm"]) > 1e-3 * ref["gradient_norm"]


# ---- A7. a large e against non-zero data -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("angle", pe.LARGE_ANGLES)
def test_a_large_error_beside_a_textured_system(angle, objective):
    """The prior sits 1.0 (2.0) rad from the start under a Lambda a thousandth of H's translation diagonal: Log runs in its
    large-angle regime in every iteration while H and g are the data's."""
    p = pe.levels_pair()
    mi = [pe.LARGE_ITER]
    prior = pe.large_prior_state(angle)
    with _engine(objective, p["K"], pe.LEVELS_W, pe.LEVELS_H, 2, mi) as eng:
        _upload(eng, [p])
        pyr = _device_pyramid(eng, 0, 1, 1, mi)
        Lam = cases.lambda_iso(pe.LARGE_WEIGHT_FRACTION * pe.finest_h00(pyr, p["K"]))
        s, reps, preps, rob = _align(eng, objective, [0], [1], [prior], [Lam], [pe.LARGE_INIT])
    ref = pr.optimize(pyr, p["K"], cases.cfg(mi), prior, Lam, robust=objective == ROBUST, init_pose=pe.LARGE_INIT)
    assert ie.flat(ref) and ref["flags"] == 0 and ref["max_angle"] >= angle - 0.1
    _compare(s[0], reps[0], preps[0], _rob(rob, 0), ref, Lam, 1)
