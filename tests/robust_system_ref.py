"""CPU checker of phovo_engine_evaluate_robust_pairs, in numpy: the weighted twist-basis system of the robust
inverse-compositional objective at the pose (R, t) = eigenPose(state), on the rows the inverse-compositional aligner defines
(tests/inverse_ref.py: rows_vectorised, and rows_loop pixel by pixel), with the median rule and the weights of
tests/inverse_robust_ref.py (median_vectorised / median_loop, weights):
  delta = scale * m at THIS state's residuals, or the caller's own (then median = 0),
  H = sum w J J^T, g = sum w J r, cost = sum w r^2, huber_cost = sum (|r| <= delta ? r^2 : 2 delta |r| - delta^2),
  squared_cost = sum r^2, rows, outliers = rows with |r| > delta.
A reference is a dict of these plus the two margins on which exact counts rest (inverse_robust_ref._margins): the distance
of |r| * 4096 from the integers 1, 2, ... in bins, and of |r| from delta.  The bars are the project's own
(sampled_system_ref.check_against for H and g, 1e-12 relative for each cost, 4 ulp for delta and median: DESIGN.md §22).
Test infrastructure, not collected."""
import numpy as np

import inverse_ref as ir
import inverse_robust_ref as rr
from inverse_robust_cases import BIN_MARGIN_FLOOR, DELTA_MARGIN_FLOOR
from sampled_system_ref import check_against

PAIR_NONFINITE, PAIR_RANK_DEFICIENT = ir.PAIR_NONFINITE, ir.PAIR_RANK_DEFICIENT
COST_BAR = 1e-12
ULPS = 4
COSTS = ("cost", "huber_cost", "squared_cost")


def _sums(r, J, rows, scale, delta, median):
    """r [n], J [n, 6] over all pixels, rows bool [n] (inverse_ref.rows_*): the record and the margins."""
    rr_ = r[rows]                                                # the rows' residuals: what the histogram and the counts see
    given = delta is not None
    if given:
        m, delta = 0.0, float(delta)
    else:
        m = median(rr_)
        delta = scale * m
    bin_margin, delta_margin = rr._margins(rr_, delta)
    if given:
        bin_margin = np.inf                                      # (no histogram is taken: no bin decides anything)
    # The sums run over ALL pixels, as inverse_system_ref's do (pixels that are no rows hold exact zeros in r and J, and a
    # zero residual has weight 1): at unit weights H, g and the squared cost are that checker's bit for bit.
    with np.errstate(all="ignore"):
        ar = np.abs(r)
        w = rr.weights(r, delta)
        Jw = J * w[:, None]
        Js = J * np.sqrt(w)[:, None]                             # H = Js^T Js: one array, so the product inverse_system_ref takes
        huber = np.where(ar <= delta, r * r, 2.0 * delta * ar - delta * delta)
        return dict(H=Js.T @ Js, g=Jw.T @ r, cost=float(np.sum(w * r * r)), huber_cost=float(np.sum(huber)),
                    squared_cost=float(np.sum(r * r)), delta=float(delta), median=float(m), rows=int(rows.sum()),
                    outliers=int(np.sum(np.abs(rr_) > delta)), last_bin=int(np.sum(rr.bins(rr_) == rr.NB - 1)),
                    bin_margin=bin_margin, delta_margin=delta_margin)


def system(planes, level, K, state, scale=rr.DEFAULT_SCALE, lo=0.3, hi=5.0, delta=None):
    """The record at `state` on planes = (i0, d0, gx0, gy0, i1) of the level, as a dict (the module's docstring)."""
    with np.errstate(all="ignore"):
        R, t = ir.eigen_rt(state)
        return _sums(*ir.rows_vectorised(planes, level, K, R, t, lo, hi), scale, delta, rr.median_vectorised)


def system_loop(planes, level, K, state, scale=rr.DEFAULT_SCALE, lo=0.3, hi=5.0, delta=None):
    """The same from inverse_ref.rows_loop and inverse_robust_ref.median_loop: one source pixel at a time (tiny images)."""
    R, t = ir.eigen_rt(state)
    return _sums(*ir.rows_loop(planes, level, K, R, t, lo, hi), scale, delta, rr.median_loop)


def flags_of(ref):
    """The record's flags: RANK_DEFICIENT below 6 rows, NONFINITE when a sum is not finite."""
    finite = np.all(np.isfinite(ref["H"])) and np.all(np.isfinite(ref["g"])) and all(np.isfinite(ref[c]) for c in COSTS)
    return (PAIR_RANK_DEFICIENT if ref["rows"] < 6 else 0) | (0 if finite else PAIR_NONFINITE)


def margins_hold(ref):
    """Exact counts (outliers, and through the bins delta itself) can be asked for only away from the bin edges and delta."""
    return ref["bin_margin"] >= BIN_MARGIN_FLOOR and ref["delta_margin"] >= DELTA_MARGIN_FLOOR


def ulps(a, b):
    """The distance of two finite doubles of one sign in units in the last place of the larger."""
    if a == b:
        return 0.0
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def _cost_close(got, want):
    return abs(got - want) <= COST_BAR * abs(want)


def check_record(rec, k, ref, given=False):
    """Record k of evaluate_robust_pairs' dict against a reference of system(): first the two margins of the reference,
    then the project's bars -- H and g by check_against, each cost within 1e-12 relative, delta and median within 4 ulp
    (a given delta echoed bit for bit, the median then 0), rows, outliers and flags exact, the matrix exactly symmetric; a
    system without rows is exactly zero.  Returns (dH / bar, dg / bar) (0, 0 where no bar applies)."""
    assert margins_hold(ref), ("margins", ref["bin_margin"], ref["delta_margin"])
    Hd, gd = rec["information"][k], rec["gradient"][k]
    assert np.array_equal(Hd, Hd.T) or not np.all(np.isfinite(Hd)), Hd
    assert rec["rows"][k] == ref["rows"], (rec["rows"][k], ref["rows"])
    if given:
        assert rec["delta"][k] == ref["delta"] and rec["median"][k] == 0.0, (rec["delta"][k], rec["median"][k])
    else:
        assert ulps(rec["delta"][k], ref["delta"]) <= ULPS, (rec["delta"][k], ref["delta"])
        assert ulps(rec["median"][k], ref["median"]) <= ULPS, (rec["median"][k], ref["median"])
    assert rec["outliers"][k] == ref["outliers"], (rec["outliers"][k], ref["outliers"])
    assert rec["flags"][k] == flags_of(ref), (rec["flags"][k], flags_of(ref))
    if ref["rows"] == 0:
        assert not Hd.any() and not gd.any() and all(rec[c][k] == 0.0 for c in COSTS)
        assert given or (rec["delta"][k] == 0.0 and rec["median"][k] == 0.0)
        return 0.0, 0.0
    H, g = ref["H"], ref["g"]
    for c in COSTS:                                              # a non-finite cost is non-finite on both sides
        if np.isfinite(ref[c]):
            assert _cost_close(rec[c][k], ref[c]), (c, rec[c][k], ref[c])
        else:
            assert not np.isfinite(rec[c][k]), (c, rec[c][k])
    if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g))):
        # the non-finite sums are non-finite on both sides, slot by slot
        assert np.array_equal(np.isfinite(Hd), np.isfinite(H)) and np.array_equal(np.isfinite(gd), np.isfinite(g))
        return 0.0, 0.0
    if not np.any(H):                                            # a constant source: every row exactly zero
        assert not Hd.any() and not gd.any()
        return 0.0, 0.0
    dh, dg = check_against(Hd, gd, rec["rows"][k], rec["cost"][k], H, g, ref["rows"], ref["cost"])
    return dh / 1e-10, dg
