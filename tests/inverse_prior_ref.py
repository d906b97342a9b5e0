"""CPU checker of the Gaussian pose prior of the two inverse-compositional objectives (phovo_engine_enqueue_align_prior,
DESIGN.md §24), in numpy, around inverse_ref (objective 5) and inverse_robust_ref (objective 6).

TEST INFRASTRUCTURE ONLY.  Rows, residual, Jacobian row, Exp, composition, termination and the level's exit are inverse_ref's;
the histogram, median rule, lag and weights are inverse_robust_ref's.  New here, in every iteration before the solve, with the
prior pose T_p = eigenPose(prior_state), the information matrix Lambda (twist order nu, omega) and the level's scale s_L:
    e  = Log(T_p^-1 T) = Log(R_p^T R, R_p^T (t - t_p))
    H' = H + s_L Lambda,   g' = g + s_L Lambda e,   xi = -lambda_L H'^-1 g'
termination and gradient_norm on ||g'||; with Lambda = 0 or s_L = 0 the two additions are skipped, so the record is
inverse_ref.optimize's (inverse_robust_ref.optimize's) bit for bit.  The record adds `error` (e at the final pose of the
finest executed level), `prior_cost` (e^T Lambda e there) and `max_angle` (the largest |omega| of any e that was formed).
`mutant` builds a deliberately wrong rule, for the tests that show the fixtures can tell: "left" takes e = Log(T T_p^-1),
"minus" subtracts s_L Lambda e, "data_norm" terminates and reports on ||g|| instead of ||g'||."""
import numpy as np

import inverse_ref as ir
import inverse_robust_ref as rr
from inverse_ref import PAIR_NONFINITE, PAIR_RANK_DEFICIENT, pose_bar  # noqa: F401

LOG_SERIES_BELOW = 1e-8      # th^2 under which Log's two factors come from their series


def se3_log(R, t):
    """The twist (nu, omega) with Exp(twist) = (R, t): w = vee(R - R^T) / 2, s = |w|, c = (tr R - 1) / 2, th = atan2(s, c),
    omega = (th / s) w, nu = (I - W / 2 + D W^2) t, D = (1 - (th / 2) cot(th / 2)) / th^2; series through th^4 below
    th^2 = 1e-8."""
    R = np.asarray(R, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        s = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        c = 0.5 * ((R[0, 0] + R[1, 1] + R[2, 2]) - 1.0)
        th = np.arctan2(s, c)
        th2 = th * th
        if th2 < LOG_SERIES_BELOW:
            k = 1.0 + th2 * (1.0 / 6.0 + th2 * (7.0 / 360.0))
            D = 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0))
        else:
            hf = 0.5 * th
            k = th / s
            D = (1.0 - hf * np.cos(hf) / np.sin(hf)) / th2
        om = k * w
        a = np.cross(om, t)
        b = np.cross(om, a)
        nu = (t - 0.5 * a) + D * b
    return np.concatenate([nu, om])


def prior_error(Rp, tp, R, t, mutant=None):
    with np.errstate(all="ignore"):
        if mutant == "left":                                   # Log(T T_p^-1): the wrong side
            Rr = R @ Rp.T
            return se3_log(Rr, t - Rr @ tp)
        return se3_log(Rp.T @ R, Rp.T @ (t - tp))


def symmetric_from_upper(information):
    """The matrix the device reads: the upper triangle of `information`, mirrored."""
    A = np.asarray(information, dtype=np.float64).reshape(6, 6)
    U = np.triu(A)
    return U + np.triu(A, 1).T


def optimize(pyr, K, cfg, prior_state, information, level_scale=None, robust=False, scale_factor=rr.DEFAULT_SCALE,
             init_pose=None, mutant=None):
    """inverse_ref.optimize (robust: inverse_robust_ref.optimize) with the prior; the same record, where cond is that of H'
    (what is solved), plus error, prior_cost, max_angle and, under `robust`, delta, outliers, bin_margin, delta_margin."""
    nl = cfg["num_levels"]
    scales = [1.0] * nl if level_scale is None else [float(v) for v in level_scale[:nl]]
    Lam = symmetric_from_upper(information)
    has_lambda = bool(np.any(Lam != 0.0))
    Rp, tp = ir.eigen_rt(prior_state)
    state = np.zeros(6) if init_pose is None else np.array(init_pose, dtype=np.float64)
    iters, valid, deltas, outl = [0] * nl, [0] * nl, [0.0] * nl, [0] * nl
    flags, gnorm, cond, margin, h_norm = 0, 0.0, 0.0, np.inf, 0.0
    bin_margin, delta_margin, max_angle = np.inf, np.inf, 0.0
    error, prior_cost = np.zeros(6), 0.0
    gate = (cfg.get("min_depth", 0.3), cfg.get("max_depth", 5.0))
    for L in range(nl - 1, -1, -1):
        if cfg["max_iter"][L] <= 0:
            iters[L] = 1
            continue
        with np.errstate(all="ignore"):
            R, t = ir.eigen_rt(state)
        if robust:
            r, _, rows = ir.rows_vectorised(pyr[L], L, K, R, t, *gate)        # the entry pass: delta_0
            bin_margin = min(bin_margin, rr._margins(r[rows])[0])
            delta = scale_factor * rr.median_vectorised(r[rows])
        it = 0
        while True:
            r, J, rows = ir.rows_vectorised(pyr[L], L, K, R, t, *gate)
            n_rows = int(rows.sum())
            if robust:
                r, J = r[rows], J[rows]
                bm, dm = rr._margins(r, delta)
                bin_margin, delta_margin = min(bin_margin, bm), min(delta_margin, dm)
                with np.errstate(all="ignore"):
                    w = rr.weights(r, delta)
                    Jw = J * w[:, None]
                    g, Hm = Jw.T @ r, Jw.T @ J
                    outl[L] = int((np.abs(r) > delta).sum())
                deltas[L] = delta
                delta = scale_factor * rr.median_vectorised(r)                # the next system's
            else:
                with np.errstate(all="ignore"):
                    g, Hm = J.T @ r, J.T @ J
            valid[L] = n_rows
            if n_rows < 6:
                flags |= PAIR_RANK_DEFICIENT
            g_data = g
            if has_lambda and scales[L] != 0.0:
                e = prior_error(Rp, tp, R, t, mutant)
                max_angle = max(max_angle, float(np.linalg.norm(e[3:]))) if np.all(np.isfinite(e)) else np.inf
                with np.errstate(all="ignore"):
                    Hm = Hm + scales[L] * Lam
                    g = g - scales[L] * (Lam @ e) if mutant == "minus" else g + scales[L] * (Lam @ e)
            try:
                with np.errstate(all="ignore"):
                    step = np.linalg.solve(Hm, g)
                    cond = max(cond, float(np.linalg.cond(Hm)))
            except np.linalg.LinAlgError:                       # an exactly singular system: the device's 1 / 0
                step = np.full(6, np.nan)
                cond = np.inf
            with np.errstate(all="ignore"):
                ER, Et = ir.se3_exp(-cfg["lam"][L] * step)
                R, t = R @ ER, R @ Et + t
            gnorm = float(np.linalg.norm(g_data if mutant == "data_norm" else g))
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
        with np.errstate(all="ignore"):
            error = prior_error(Rp, tp, R, t)
            prior_cost = float(error @ (Lam @ error)) if has_lambda else 0.0
        state = ir.state_from_pose(R, t) if finite else np.full(6, np.nan)
    rec = dict(state=state, iterations=iters, valid_pixels=valid, flags=flags, gradient_norm=gnorm, cond=cond,
               margin=margin, h_norm=h_norm, error=error, prior_cost=prior_cost, max_angle=max_angle)
    if robust:
        rec.update(delta=deltas, outliers=outl, bin_margin=bin_margin, delta_margin=delta_margin)
    return rec
