"""CPU checker of the affine-illumination objective (PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE), in numpy.

TEST INFRASTRUCTURE ONLY.  The rows are the bilinear-corrected rows of oracle/numpy_twin.py -- the vectorised form below
calls numpy_twin.normal_equations_bilinear(corrected=True) for them -- with the residual
    r_k = I1(u_k, v_k) - (1 + alpha) I0_k - beta
and two columns appended, dr/dalpha = -I0_k and dr/dbeta = -1.  The state has 8 entries (x, y, z, yaw, pitch, roll, alpha,
beta).  rows_loop is the same definition written out pixel by pixel, for tiny images; optimize is the level loop (the twin's
optimize() with 8 in place of 6, numpy.linalg.solve) and records, per accepted state, cond(J^T J) and how close ||g|| came
to min_gradient_norm."""
import numpy as np

from oracle import numpy_twin as twin

PAIR_NONFINITE, PAIR_RANK_DEFICIENT = 1, 4
NP = 8


def rows_vectorised(planes, level, K, state8, min_depth=0.3, max_depth=5.0):
    """planes = (i0, d0, i1, gx1, gy1) of the level.  Returns (r[N], J[N,8], rows[N] bool); rows outside are zero."""
    i0, d0, i1, gx1, gy1 = planes
    pose, alpha, beta = np.asarray(state8[:6], dtype=np.float64), float(state8[6]), float(state8[7])
    res, J6 = twin.normal_equations_bilinear(planes, level, K, pose, min_depth, max_depth, corrected=True)
    # which pixels are rows: the twin's own gate and bounds test, read off a run on I0 = 0, I1 = 1, whose residual is
    # the bilinear sample of a plane of ones (1 up to rounding) on every row and 0 elsewhere
    z, o = np.zeros_like(i0), np.ones_like(i0)
    probe, _ = twin.normal_equations_bilinear((z, d0, o, z, z), level, K, pose, min_depth, max_depth, corrected=True)
    rows = probe != 0.0
    i0f = i0.reshape(-1)
    # res = I1(u, v) - I0 on the rows; the gain and offset act on the source intensity
    r = np.where(rows, res - alpha * i0f - beta, 0.0)
    J = np.zeros((i0f.size, NP))
    J[:, :6] = J6
    J[rows, 6] = -i0f[rows]
    J[rows, 7] = -1.0
    return r, J, rows


def rows_loop(planes, level, K, state8, min_depth=0.3, max_depth=5.0):
    """The same rows, one source pixel at a time in raster order (tiny images).  Also returns, per row, which clamp band
    its taps fell in: 'c-' / 'c+' / 'r-' / 'r+' (a tap column / row clamped at the low / high edge)."""
    i0, d0, i1, gx1, gy1 = planes
    H, W = i0.shape
    sf = 1.0 / 2 ** level
    fx, fy, ox, oy = K[0, 0] * sf, K[1, 1] * sf, K[0, 2] * sf, K[1, 2] * sf
    x, y, z, yaw, pitch, roll, alpha, beta = [float(v) for v in state8]
    sy, cy, sp, cp, sr, cr = np.sin(yaw), np.cos(yaw), np.sin(pitch), np.cos(pitch), np.sin(roll), np.cos(roll)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    n = H * W
    r = np.zeros(n)
    J = np.zeros((n, NP))
    rows = np.zeros(n, dtype=bool)
    bands = {}
    stats = dict(gate=0, oob=0)
    for k in range(n):
        rr, cc = divmod(k, W)
        pz = d0[rr, cc]
        if not (min_depth < pz < max_depth):                     # depth gate (NaN fails)
            stats["gate"] += 1
            continue
        px = (cc - ox) * pz / fx
        py = (rr - oy) * pz / fy
        P = R @ np.array([px, py, pz]) + np.array([x, y, z])
        iz = 1.0 / P[2]
        tc, tr = P[0] * fx * iz + ox, P[1] * fy * iz + oy
        if not (tc > -0.5 and tc < W - 0.5 and tr > -0.5 and tr < H - 0.5):      # in bounds iff the nearest pixel is
            stats["oob"] += 1
            continue
        fc, fr = np.floor(tc), np.floor(tr)
        ax, ay = tc - fc, tr - fr
        c0, c1 = int(min(max(fc, 0), W - 1)), int(min(max(fc + 1, 0), W - 1))
        r0, r1 = int(min(max(fr, 0), H - 1)), int(min(max(fr + 1, 0), H - 1))
        band = set()
        if fc < 0: band.add("c-")
        if fc + 1 > W - 1: band.add("c+")
        if fr < 0: band.add("r-")
        if fr + 1 > H - 1: band.add("r+")
        bands[k] = band

        def smp(Pl):
            return (1 - ay) * ((1 - ax) * Pl[r0, c0] + ax * Pl[r0, c1]) + ay * ((1 - ax) * Pl[r1, c0] + ax * Pl[r1, c1])
        gxs, gys = smp(gx1), smp(gy1)
        # the true derivative of the projection: d(u, v) / d(x, y, z, yaw, pitch, roll)
        Xr, Yr, Zr = P[0] - x, P[1] - y, P[2] - z
        dP = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]),
              np.array([-Yr, Xr, 0.0]),
              np.array([cy * Zr, sy * Zr, -(cp * px + sp * sr * py + sp * cr * pz)]),
              np.array([R[0, 2] * py - R[0, 1] * pz, R[1, 2] * py - R[1, 1] * pz, R[2, 2] * py - R[2, 1] * pz])]
        for j in range(6):
            du = fx * dP[j][0] * iz - fx * P[0] * dP[j][2] * iz ** 2
            dv = fy * dP[j][1] * iz - fy * P[1] * dP[j][2] * iz ** 2
            J[k, j] = gxs * du + gys * dv
        J[k, 6] = -i0[rr, cc]
        J[k, 7] = -1.0
        r[k] = smp(i1) - (1.0 + alpha) * i0[rr, cc] - beta
        rows[k] = True
    return r, J, rows, bands, stats


def system(planes, level, K, state8, min_depth=0.3, max_depth=5.0):
    """(g[8], H[8,8], number of rows) at the state."""
    with np.errstate(all="ignore"):
        r, J, rows = rows_vectorised(planes, level, K, state8, min_depth, max_depth)
    return J.T @ r, J.T @ J, int(rows.sum())


def optimize(pyr, K, cfg, init_pose=None):
    """pyr[L] = (i0, d0, i1, gx1, gy1); cfg: dict(num_levels, lam, max_iter, min_grad[, min_depth, max_depth]).
    The bilinear extension's level loop with 8 in place of 6: every pair starts at alpha = beta = 0, both carry from level
    to level with the pose; per iteration x <- x - lambda_L H^-1 g, the level ends when the iteration count is reached or
    ||g||_2 (all 8 entries) < min_gradient_norm[L], tested after the step; a state that is not finite ends the level too.
    Levels with max_num_iterations 0 are skipped (they report one iteration, like the photometric objective's).
    Returns dict(state[8], iterations[L], valid_pixels[L], flags, gradient_norm, cond, margin, h_norm):
      cond     the largest cond(J^T J) over the states the loop accepted (inf: a singular system)
      margin   the smallest |  ||g|| - min_gradient_norm | / min_gradient_norm over all iterations (inf with thresholds 0)
      h_norm   ||H||_2 of the system gradient_norm belongs to (inf where H is not finite): a state difference e moves that
               gradient norm by at most h_norm |e| to first order
      noise_level  the first level (the coarsest such) with an iteration of 1 ... 7 rows, or None.  J^T J then has rank below
               8 without being exactly zero: unless a pivot is an exact zero (a black source), its last pivots are rounding
               noise on the device and here alike, and nothing after that step is defined."""
    nl = cfg["num_levels"]
    state = np.zeros(NP)
    if init_pose is not None:
        state[:6] = np.asarray(init_pose, dtype=np.float64)
    iters, valid = [0] * nl, [0] * nl
    flags, gnorm, cond, margin, h_norm, noise_level = 0, 0.0, 0.0, np.inf, 0.0, None
    for L in range(nl - 1, -1, -1):
        if cfg["max_iter"][L] <= 0:
            iters[L] = 1
            continue
        it = 0
        while True:
            g, Hm, n_rows = system(pyr[L], L, K, state, cfg.get("min_depth", 0.3), cfg.get("max_depth", 5.0))
            valid[L] = n_rows
            if n_rows < NP:
                flags |= PAIR_RANK_DEFICIENT
                if n_rows > 0 and noise_level is None:
                    noise_level = L
            try:
                with np.errstate(all="ignore"):
                    step = np.linalg.solve(Hm, g)
                    cond = max(cond, float(np.linalg.cond(Hm)))
            except np.linalg.LinAlgError:                       # an exactly singular system: the device's 1 / 0
                step = np.full(NP, np.nan)
                cond = np.inf
            state = state - cfg["lam"][L] * step
            gnorm = float(np.linalg.norm(g))
            h_norm = float(np.linalg.norm(Hm, 2)) if np.all(np.isfinite(Hm)) else np.inf
            thr = cfg["min_grad"][L]
            if thr > 0:
                margin = min(margin, abs(gnorm - thr) / thr)
            it += 1
            finite = bool(np.all(np.isfinite(state)))
            if not finite:
                flags |= PAIR_NONFINITE
            if it >= cfg["max_iter"][L] or gnorm < thr or not finite:
                break
        iters[L] = it
    return dict(state=state, iterations=iters, valid_pixels=valid, flags=flags, gradient_norm=gnorm, cond=cond,
                margin=margin, h_norm=h_norm, noise_level=noise_level)


def pose_bar(cond, states, flat=1e-9):
    """The project's parity bar flat x max(1, |x|), widened where the checker's cond(J^T J) exceeds what the flat bar
    assumes exactly as conditioned_allowance (tests/tools/fuzz_objectives.py) does: x max(1, cond / 1e5), capped at 1e-5."""
    return min(1e-5, flat * max(1.0, cond / 1e5)) * max(1.0, float(np.abs(states).max()))
