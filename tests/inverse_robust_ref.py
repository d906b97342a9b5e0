"""CPU checker of the robust inverse-compositional objective (PHOVO_OBJECTIVE_INVERSE_ROBUST), in numpy, on
inverse_ref's rows.

TEST INFRASTRUCTURE ONLY.  Rows, residual, Jacobian row, Exp, composition and the level's exit are inverse_ref's.  New here:
  bins      q = |r| * 4096, bin = int(q) where q < 4096, else 4095 (|r| >= 1 and NaN),
  median    n rows, half = (n + 1) // 2, k the first bin whose cumulative count reaches half, `before` the count below it,
            m = (k + (half - before) / h[k]) * 2^-12, and 0 for n = 0,
  delta     scale_factor * m, lagging: delta_0 from the residuals at the level's entry pose, delta_{i+1} from iteration i's,
  weights   w = 1 where |r| <= delta_i, else delta_i / |r|;  H = sum w J J^T, g = sum w J r;  outliers = rows with |r| > delta_i.
median_loop is the same median rule written out residual by residual, for tiny inputs.  optimize also records how close the
fixture comes to the places where rounding could move a COUNT: the distance of |r| * 4096 from the integers from 1 up
(`bin_margin`, in bins) and of |r| from the delta it is compared with (`delta_margin`)."""
import numpy as np

import inverse_ref as ir
from inverse_ref import PAIR_NONFINITE, PAIR_RANK_DEFICIENT, pose_bar  # noqa: F401

NB = 4096
DEFAULT_SCALE = 1.345 * 1.4826


def bins(r):
    """The bin of every residual."""
    with np.errstate(all="ignore"):
        q = np.abs(np.asarray(r, dtype=np.float64)) * 4096.0
        inside = q < 4096.0
        return np.where(inside, np.where(inside, q, 0.0).astype(np.int64), NB - 1)


def median_rule(h):
    """m of a histogram h[4096] of counts."""
    n = int(h.sum())
    if n == 0:
        return 0.0
    half = (n + 1) // 2
    cum = np.cumsum(h)
    k = int(np.searchsorted(cum, half, side="left"))
    before = int(cum[k - 1]) if k > 0 else 0
    return (float(k) + float(half - before) / float(h[k])) * 2.0 ** -12


def median_vectorised(r):
    return median_rule(np.bincount(bins(r), minlength=NB))


def median_loop(r):
    """The same, one residual at a time and one bin at a time."""
    h = [0] * NB
    n = 0
    for v in r:
        q = abs(float(v)) * 4096.0
        h[int(q) if q < 4096.0 else NB - 1] += 1
        n += 1
    if n == 0:
        return 0.0
    half = (n + 1) // 2
    before = 0
    for k in range(NB):
        if before + h[k] >= half:
            return (float(k) + float(half - before) / float(h[k])) * 2.0 ** -12
        before += h[k]
    raise AssertionError("unreachable: the counts add up to n")


def weights(r, delta):
    with np.errstate(all="ignore"):
        ar = np.abs(r)
        return np.where(ar <= delta, 1.0, delta / ar)


def _margins(r, delta=None):
    """(distance of |r| * 4096 from the integers 1, 2, ..., in bins; distance of |r| from delta), over the finite residuals."""
    ar = np.abs(r[np.isfinite(r)])
    if ar.size == 0:
        return np.inf, np.inf
    q = ar * 4096.0
    near = np.maximum(np.rint(q), 1.0)
    return float(np.abs(q - near).min()), (np.inf if delta is None else float(np.abs(ar - delta).min()))


def optimize(pyr, K, cfg, scale_factor=DEFAULT_SCALE, init_pose=None):
    """inverse_ref.optimize's loop and record under the robust weights, plus delta[L] and outliers[L] of every level's last
    system, bin_margin and delta_margin (see the module's docstring)."""
    nl = cfg["num_levels"]
    state = np.zeros(6) if init_pose is None else np.array(init_pose, dtype=np.float64)
    iters, valid, deltas, outl = [0] * nl, [0] * nl, [0.0] * nl, [0] * nl
    flags, gnorm, cond, margin, h_norm = 0, 0.0, 0.0, np.inf, 0.0
    bin_margin, delta_margin = np.inf, np.inf
    gate = (cfg.get("min_depth", 0.3), cfg.get("max_depth", 5.0))
    for L in range(nl - 1, -1, -1):
        if cfg["max_iter"][L] <= 0:
            iters[L] = 1
            continue
        with np.errstate(all="ignore"):
            R, t = ir.eigen_rt(state)
        r, _, rows = ir.rows_vectorised(pyr[L], L, K, R, t, *gate)            # the entry pass: delta_0
        bin_margin = min(bin_margin, _margins(r[rows])[0])
        delta = scale_factor * median_vectorised(r[rows])
        it = 0
        while True:
            r, J, rows = ir.rows_vectorised(pyr[L], L, K, R, t, *gate)
            r, J = r[rows], J[rows]
            n_rows = int(rows.sum())
            bm, dm = _margins(r, delta)
            bin_margin, delta_margin = min(bin_margin, bm), min(delta_margin, dm)
            with np.errstate(all="ignore"):
                w = weights(r, delta)
                Jw = J * w[:, None]
                g, Hm = Jw.T @ r, Jw.T @ J
                outl[L] = int((np.abs(r) > delta).sum())
            deltas[L] = delta
            delta = scale_factor * median_vectorised(r)                       # the next system's
            valid[L] = n_rows
            if n_rows < 6:
                flags |= PAIR_RANK_DEFICIENT
            try:
                with np.errstate(all="ignore"):
                    step = np.linalg.solve(Hm, g)
                    cond = max(cond, float(np.linalg.cond(Hm)))
            except np.linalg.LinAlgError:
                step = np.full(6, np.nan)
                cond = np.inf
            with np.errstate(all="ignore"):
                ER, Et = ir.se3_exp(-cfg["lam"][L] * step)
                R, t = R @ ER, R @ Et + t
            gnorm = float(np.linalg.norm(g))
            h_norm = float(np.linalg.norm(Hm, 2)) if np.all(np.isfinite(Hm)) else np.inf
            thr = cfg["min_grad"][L]
            if thr > 0:
                margin = min(margin, abs(gnorm - thr) / thr)
            it += 1
            finite = bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t)))
            if not finite:
                flags |= PAIR_NONFINITE
            if it >= cfg["max_iter"][L] or gnorm < thr or not finite:
                break
        iters[L] = it
        state = ir.state_from_pose(R, t) if finite else np.full(6, np.nan)
    return dict(state=state, iterations=iters, valid_pixels=valid, flags=flags, gradient_norm=gnorm, cond=cond,
                margin=margin, h_norm=h_norm, delta=deltas, outliers=outl, bin_margin=bin_margin,
                delta_margin=delta_margin)
