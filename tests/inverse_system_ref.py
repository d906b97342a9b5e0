"""CPU checker of phovo_engine_evaluate_inverse_pairs, in numpy: H = sum J J^T, g = sum J r, cost = sum r^2
and the row count of the rows the inverse-compositional aligner defines (tests/inverse_ref.py: rows_vectorised, and
rows_loop pixel by pixel) at the pose (R, t) = eigenPose(state), in the twist basis (nu, omega).  The bars are the project's
own (sampled_system_ref.check_against).  Test infrastructure, not collected."""
import numpy as np

import inverse_ref as ir
from sampled_system_ref import check_against  # noqa: F401

PAIR_NONFINITE, PAIR_RANK_DEFICIENT = ir.PAIR_NONFINITE, ir.PAIR_RANK_DEFICIENT


def _sums(r, J, rows):
    with np.errstate(all="ignore"):                              # (pixels that are no rows hold exact zeros: inverse_ref.system's sums)
        return J.T @ J, J.T @ r, float(np.sum(r * r)), int(rows.sum())


def system(planes, level, K, state, lo=0.3, hi=5.0):
    """(H[6,6], g[6], cost, rows) at `state` on planes = (i0, d0, gx0, gy0, i1) of the level."""
    with np.errstate(all="ignore"):
        R, t = ir.eigen_rt(state)
        return _sums(*ir.rows_vectorised(planes, level, K, R, t, lo, hi))


def system_loop(planes, level, K, state, lo=0.3, hi=5.0):
    """The same from inverse_ref.rows_loop: one source pixel at a time (tiny images)."""
    R, t = ir.eigen_rt(state)
    return _sums(*ir.rows_loop(planes, level, K, R, t, lo, hi))


def flags_of(H, g, cost, rows):
    """The record's flags: RANK_DEFICIENT below 6 rows, NONFINITE when a sum is not finite."""
    finite = np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.isfinite(cost)
    return (PAIR_RANK_DEFICIENT if rows < 6 else 0) | (0 if finite else PAIR_NONFINITE)


def sampled_target_pixels(planes, level, K, state, lo=0.3, hi=5.0):
    """bool[H, W]: the pixels of I1 that a row reads -- all four clamped taps of every row, those of weight 0 included
    (0 x NaN is NaN)."""
    i0, d0, _, _, _ = planes
    h, w = i0.shape
    fx, fy, ox, oy = ir._intrinsics(level, K)
    R, t = ir.eigen_rt(state)
    _, _, rows = ir.rows_vectorised(planes, level, K, R, t, lo, hi)
    cc, rr = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    pz = d0.reshape(-1)
    hit = np.zeros((h, w), dtype=bool)
    with np.errstate(all="ignore"):
        P = R @ np.stack([(cc.reshape(-1) - ox) * pz / fx, (rr.reshape(-1) - oy) * pz / fy, pz]) + t.reshape(3, 1)
        tc, tr = P[0] * fx / P[2] + ox, P[1] * fy / P[2] + oy
    fc, fr = np.floor(tc[rows]), np.floor(tr[rows])
    for dc in (0, 1):
        for dr in (0, 1):
            hit[np.clip(fr + dr, 0, h - 1).astype(int), np.clip(fc + dc, 0, w - 1).astype(int)] = True
    return hit


def check_record(rec, k, ref):
    """Record k of evaluate_inverse_pairs' dict against ref = (H, g, cost, rows): the project's bars, flags exact, the
    matrix exactly symmetric; a system without rows is exactly zero.  Returns (dH / bar, dg / bar) (0, 0 where no bar applies)."""
    H, g, cost, rows = ref
    Hd = rec["information"][k]
    assert np.array_equal(Hd, Hd.T) or not np.all(np.isfinite(Hd)), Hd
    assert rec["rows"][k] == rows, (rec["rows"][k], rows)
    assert rec["flags"][k] == flags_of(H, g, cost, rows), (rec["flags"][k], flags_of(H, g, cost, rows))
    if rows == 0:
        assert rec["cost"][k] == 0.0 and not Hd.any() and not rec["gradient"][k].any()
        return 0.0, 0.0
    if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g))):
        # the non-finite sums are non-finite on both sides, slot by slot; the cost keeps its bar where it is finite
        assert np.array_equal(np.isfinite(Hd), np.isfinite(H)) and np.array_equal(np.isfinite(rec["gradient"][k]), np.isfinite(g))
        if np.isfinite(cost):
            assert abs(rec["cost"][k] - cost) <= 1e-12 * abs(cost), (rec["cost"][k], cost)
        return 0.0, 0.0
    if not np.any(H):                                            # a constant source: every row exactly zero
        assert not Hd.any() and not rec["gradient"][k].any()
        assert abs(rec["cost"][k] - cost) <= 1e-12 * abs(cost), (rec["cost"][k], cost)
        return 0.0, 0.0
    dh, dg = check_against(Hd, rec["gradient"][k], rec["rows"][k], rec["cost"][k], H, g, rows, cost)
    return dh / 1e-10, dg
