"""CPU checker of the inverse-compositional objective (PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL), in numpy.

TEST INFRASTRUCTURE ONLY.  The rows are the bilinear extension's (oracle/numpy_twin.normal_equations_bilinear: depth gate,
real-valued warp, in bounds iff the nearest pixel is, four clamped taps of I1, r = I1(u, v) - I0), written here for a pose
given as (R, t); the Jacobian row is taken on the source side,
    a = (gx0 fx / pz, gy0 fy / pz, -(a_0 px + a_1 py) / pz),   J = (a, p x a)          (twist order: nu, omega),
and the step is composed on SE(3): xi = -lambda H^-1 g, (R, t) <- (R E_R, R E_t + t), (E_R, E_t) = Exp(xi).
rows_loop is the same definition written out pixel by pixel, for tiny images; optimize is the level loop and records, per
accepted pose, cond(J^T J) and how close ||g|| came to min_gradient_norm (affine_ref.optimize's record)."""
import numpy as np

from affine_ref import pose_bar  # noqa: F401  (the same rule: flat 1e-9 x max(1, |x|), widened by conditioning)

PAIR_NONFINITE, PAIR_RANK_DEFICIENT = 1, 4
TAYLOR_BELOW = 1e-8          # |omega|^2 under which Exp's coefficients come from their series


def eigen_rt(state):
    """eigenPose(state) as (R[3,3], t[3]): R = Rz(yaw) Ry(pitch) Rx(roll)."""
    x, y, z, yaw, pitch, roll = [float(v) for v in state]
    sy, cy, sp, cp, sr, cr = np.sin(yaw), np.cos(yaw), np.sin(pitch), np.cos(pitch), np.sin(roll), np.cos(roll)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return R, np.array([x, y, z])


def state_from_pose(R, t):
    """The inverse of eigenPose wherever cos(pitch) != 0: (t, yaw, pitch, roll)."""
    yaw = np.arctan2(R[1, 0], R[0, 0])
    pitch = np.arctan2(-R[2, 0], np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0]))
    roll = np.arctan2(R[2, 1], R[2, 2])
    return np.array([t[0], t[1], t[2], yaw, pitch, roll])


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """(E_R, E_t) = Exp(xi), xi = (nu, omega): E_R = I + A W + B W^2, E_t = (I + B W + C W^2) nu, W = [omega]x,
    A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3; for th^2 < 1e-8 their Taylor series through th^4."""
    xi = np.asarray(xi, dtype=np.float64)
    nu, w = xi[:3], xi[3:]
    th2 = float(w @ w)
    if th2 < TAYLOR_BELOW:
        A = 1.0 - th2 * (1.0 / 6.0 - th2 * (1.0 / 120.0))
        B = 0.5 - th2 * (1.0 / 24.0 - th2 * (1.0 / 720.0))
        Cc = 1.0 / 6.0 - th2 * (1.0 / 120.0 - th2 * (1.0 / 5040.0))
    else:
        th = np.sqrt(th2)
        A = np.sin(th) / th
        sh = np.sin(0.5 * th)
        B = 2.0 * sh * sh / th2                 # (1 - cos th) / th^2 without the cancellation: E_t has B W nu, first order in th
        Cc = (1.0 - A) / th2
    W2 = np.outer(w, w) - th2 * np.eye(3)
    Wm = hat(w)
    ER = np.eye(3) + A * Wm + B * W2
    V = np.eye(3) + B * Wm + Cc * W2
    return ER, V @ nu


def _intrinsics(level, K):
    sf = 1.0 / 2 ** level
    return K[0, 0] * sf, K[1, 1] * sf, K[0, 2] * sf, K[1, 2] * sf


def rows_vectorised(planes, level, K, R, t, min_depth=0.3, max_depth=5.0):
    """planes = (i0, d0, gx0, gy0, i1) of the level.  Returns (r[N], J[N,6], rows[N] bool); rows outside are zero."""
    i0, d0, gx0, gy0, i1 = planes
    H_, W_ = i0.shape
    fx, fy, ox, oy = _intrinsics(level, K)
    cc, rr = np.meshgrid(np.arange(W_, dtype=np.float64), np.arange(H_, dtype=np.float64))
    pz = d0.reshape(-1)
    with np.errstate(all="ignore"):
        valid = (min_depth < pz) & (pz < max_depth)
        px = (cc.reshape(-1) - ox) * pz / fx
        py = (rr.reshape(-1) - oy) * pz / fy
        P = R @ np.stack([px, py, pz]) + np.asarray(t, dtype=np.float64).reshape(3, 1)
        iz = 1.0 / P[2]
        tc, tr = P[0] * fx * iz + ox, P[1] * fy * iz + oy
        rows = valid & (tc > -0.5) & (tc < W_ - 0.5) & (tr > -0.5) & (tr < H_ - 0.5)
        tc, tr = np.where(rows, tc, 0.0), np.where(rows, tr, 0.0)
        fc, fr = np.floor(tc), np.floor(tr)
        ax, ay = tc - fc, tr - fr
        c0, c1 = np.clip(fc, 0, W_ - 1).astype(np.int64), np.clip(fc + 1, 0, W_ - 1).astype(np.int64)
        r0, r1 = np.clip(fr, 0, H_ - 1).astype(np.int64), np.clip(fr + 1, 0, H_ - 1).astype(np.int64)
        smp = (1 - ay) * ((1 - ax) * i1[r0, c0] + ax * i1[r0, c1]) + ay * ((1 - ax) * i1[r1, c0] + ax * i1[r1, c1])
        res = smp - i0.reshape(-1)
        a0 = gx0.reshape(-1) * fx / pz
        a1 = gy0.reshape(-1) * fy / pz
        a2 = -(a0 * px + a1 * py) / pz
        J = np.stack([a0, a1, a2, py * a2 - pz * a1, pz * a0 - px * a2, px * a1 - py * a0], axis=1)
    J[~rows] = 0.0
    return np.where(rows, res, 0.0), J, rows


def rows_loop(planes, level, K, R, t, min_depth=0.3, max_depth=5.0):
    """The same rows, one source pixel at a time in raster order (tiny images)."""
    i0, d0, gx0, gy0, i1 = planes
    H, W = i0.shape
    fx, fy, ox, oy = _intrinsics(level, K)
    n = H * W
    r = np.zeros(n)
    J = np.zeros((n, 6))
    rows = np.zeros(n, dtype=bool)
    for k in range(n):
        rr, cc = divmod(k, W)
        pz = d0[rr, cc]
        if not (min_depth < pz < max_depth):                     # depth gate (NaN fails)
            continue
        p = np.array([(cc - ox) * pz / fx, (rr - oy) * pz / fy, pz])
        P = R @ p + t
        u, v = P[0] * fx / P[2] + ox, P[1] * fy / P[2] + oy
        if not (u > -0.5 and u < W - 0.5 and v > -0.5 and v < H - 0.5):          # in bounds iff the nearest pixel is
            continue
        fc, fr = np.floor(u), np.floor(v)
        ax, ay = u - fc, v - fr
        c0, c1 = int(min(max(fc, 0), W - 1)), int(min(max(fc + 1, 0), W - 1))
        r0, r1 = int(min(max(fr, 0), H - 1)), int(min(max(fr + 1, 0), H - 1))
        smp = (1 - ay) * ((1 - ax) * i1[r0, c0] + ax * i1[r0, c1]) + ay * ((1 - ax) * i1[r1, c0] + ax * i1[r1, c1])
        a = np.array([gx0[rr, cc] * fx / pz, gy0[rr, cc] * fy / pz, 0.0])
        a[2] = -(a[0] * p[0] + a[1] * p[1]) / pz
        J[k, :3] = a
        J[k, 3:] = np.cross(p, a)
        r[k] = smp - i0[rr, cc]
        rows[k] = True
    return r, J, rows


def system(planes, level, K, R, t, min_depth=0.3, max_depth=5.0):
    """(g[6], H[6,6], number of rows) at the pose (R, t), in the twist basis."""
    r, J, rows = rows_vectorised(planes, level, K, R, t, min_depth, max_depth)
    with np.errstate(all="ignore"):
        return J.T @ r, J.T @ J, int(rows.sum())


def optimize(pyr, K, cfg, init_pose=None):
    """pyr[L] = (i0, d0, gx0, gy0, i1); cfg: dict(num_levels, lam, max_iter, min_grad[, min_depth, max_depth]).
    Per level: (R, t) = eigenPose(state); per iteration xi = -lambda_L H^-1 g composed as above; the level ends after the
    step when the iteration count is reached or ||g||_2 < min_gradient_norm[L] (g in the twist basis), or when (R, t) is
    not finite; then state = state_from_pose(R, t), all NaN when (R, t) is not finite.  Levels with max_num_iterations 0
    are skipped (they report one iteration, like the photometric objective's).
    Returns affine_ref.optimize's record: dict(state[6], iterations[L], valid_pixels[L], flags, gradient_norm, cond,
    margin, h_norm)."""
    nl = cfg["num_levels"]
    state = np.zeros(6) if init_pose is None else np.array(init_pose, dtype=np.float64)
    iters, valid = [0] * nl, [0] * nl
    flags, gnorm, cond, margin, h_norm = 0, 0.0, 0.0, np.inf, 0.0
    for L in range(nl - 1, -1, -1):
        if cfg["max_iter"][L] <= 0:
            iters[L] = 1
            continue
        with np.errstate(all="ignore"):
            R, t = eigen_rt(state)
        it = 0
        while True:
            g, Hm, n_rows = system(pyr[L], L, K, R, t, cfg.get("min_depth", 0.3), cfg.get("max_depth", 5.0))
            valid[L] = n_rows
            if n_rows < 6:
                flags |= PAIR_RANK_DEFICIENT
            try:
                with np.errstate(all="ignore"):
                    step = np.linalg.solve(Hm, g)
                    cond = max(cond, float(np.linalg.cond(Hm)))
            except np.linalg.LinAlgError:                       # an exactly singular system: the device's 1 / 0
                step = np.full(6, np.nan)
                cond = np.inf
            with np.errstate(all="ignore"):
                ER, Et = se3_exp(-cfg["lam"][L] * step)
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
        state = state_from_pose(R, t) if finite else np.full(6, np.nan)
    return dict(state=state, iterations=iters, valid_pixels=valid, flags=flags, gradient_norm=gnorm, cond=cond,
                margin=margin, h_norm=h_norm)
