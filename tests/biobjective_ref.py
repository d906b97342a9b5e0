"""CPU checker of the bi-objective (intensity + depth) aligner, phovo::Analytic::CPhotoconsistencyOdometryBiObjective
(phovo/include/CPhotoconsistencyOdometryBiObjective.h).  Test infrastructure, not collected as tests.

It restates the reference's behaviour (line numbers cite that header) on top of the oracle's pyramid functions:
  (a) literal_system        the per-pixel loop of ComputeResidualsAndJacobians (:242-450) for tiny images, writing a
                            dense r[2N] and J[2N x 6] in the reference's write order (last writer wins);
  (b) normal_equations      H = J^T J and g = J^T r from the owner map and the row-resolution rule, with
                            counters of each resolution branch;
  (c) optimize              the Gauss-Newton loop of Optimize() (:587-648) with the analytic termination test.
"""
import numpy as np

from oracle import oracle


def level_intrinsics(K, level):
    sf = 1.0 / 2 ** level                                                    # :257
    fx, fy, ox, oy = K[0][0] * sf, K[1][1] * sf, K[0][2] * sf, K[1][2] * sf    # :258-261
    return fx, fy, ox, oy, 1.0 / fx, 1.0 / fy                                # :262-263


def _trig(state):
    x, y, z, yaw, pitch, roll = [float(v) for v in state]
    return x, y, z, np.sin(yaw), np.cos(yaw), np.sin(pitch), np.cos(pitch), np.sin(roll), np.cos(roll)


def rotation(state):
    """Rt (:273-295)."""
    x, y, z, sy, cy, sp, cp, sr, cr = _trig(state)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return R, np.array([x, y, z])


def target_planes(gray1, depth1, cfg, max_depth):
    """SetTargetFrame (:566-578): intensity pyramid and gradients, the depth pyramid (no blur), the depth gradients
    (BuildDepthDerivativesPyramids :214-240: Scharr of depth * (1.0/max_depth)) and the per-level gain (:300)."""
    i1p, gxp, gyp = oracle.build_target_pyramids(gray1, cfg)
    _, d1p = oracle.build_source_pyramids(gray1, depth1, cfg)
    dgxp, dgyp, gains = [], [], []
    for level in range(cfg.num_levels):
        dgx, dgy = oracle.scharr(d1p[level] * (1.0 / max_depth), cfg.image_gradients_scaling_factor[level])
        dgxp.append(dgx)
        dgyp.append(dgy)
        gains.append(np.mean(i1p[level]) / np.mean(d1p[level]))
    return dict(i1=i1p, d1=d1p, gx=gxp, gy=gyp, dgx=dgxp, dgy=dgyp, gain=gains)


def _jacobian_rt(px, py, pz, state):
    """jacobianRt (:354-384), 3 x 6 per pixel: arrays [..., 3, 6]."""
    _, _, _, sy, cy, sp, cp, sr, cr = _trig(state)
    z0, o1 = np.zeros_like(px), np.ones_like(px)
    row0 = [o1, z0, z0,
            py * (-sp * sr * sy - cr * cy) + pz * (sr * cy - sp * cr * sy) - cp * px * sy,
            cp * py * sr * cy + cp * pz * cr * cy - sp * px * cy,
            py * (sr * sy + sp * cr * cy) + pz * (cr * sy - sp * sr * cy)]
    row1 = [z0, o1, z0,
            pz * (sr * sy + sp * cr * cy) + py * (sp * sr * cy - cr * sy) + cp * px * cy,
            cp * py * sr * sy + cp * pz * cr * sy - sp * px * sy,
            pz * (-sp * sr * sy - cr * cy) + py * (sp * cr * sy - sr * cy)]
    row2 = [z0, z0, o1, z0,
            -sp * py * sr - sp * pz * cr - cp * px,
            cp * py * cr - cp * pz * sr]
    return np.stack([np.stack(row0, -1), np.stack(row1, -1), np.stack(row2, -1)], -2)


def warp(d0, level, K, state, min_depth, max_depth):
    """Depth gate (:311), unprojection (:313-314), Rt (:322), projection (:325-327), C round (:328-329), bounds
    (:333-334).  Returns per source pixel: contributes, target index (-1 where not), and the geometry for the
    Jacobians."""
    h, w = d0.shape
    fx, fy, ox, oy, ifx, ify = level_intrinsics(K, level)
    rr, cc = np.mgrid[0:h, 0:w]
    rr, cc = rr.ravel().astype(np.float64), cc.ravel().astype(np.float64)
    pz = d0.ravel().astype(np.float64)
    R, t = rotation(state)
    with np.errstate(all="ignore"):
        valid = (min_depth < pz) & (pz < max_depth)
        px = (cc - ox) * pz * ifx
        py = (rr - oy) * pz * ify
        X = R[0, 0] * px + R[0, 1] * py + R[0, 2] * pz + t[0]
        Y = R[1, 0] * px + R[1, 1] * py + R[1, 2] * pz + t[1]
        Z = R[2, 0] * px + R[2, 1] * py + R[2, 2] * pz + t[2]
        iz = 1.0 / Z
        tc = (X * fx) * iz + ox
        tr = (Y * fy) * iz + oy
        tri, tci = oracle_round(tr), oracle_round(tc)
        contrib = valid & (tri >= 0) & (tri < h) & (tci >= 0) & (tci < w)
    tgt = np.full(h * w, -1, dtype=np.int64)
    tgt[contrib] = (tri[contrib] * w + tci[contrib]).astype(np.int64)
    return dict(contrib=contrib, tgt=tgt, px=px, py=py, pz=pz, X=X, Y=Y, iz=iz, fx=fx, fy=fy)


def oracle_round(v):
    """C round(): half away from zero."""
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def jacobians(wp, gx, gy, dgx, dgy, gain, state):
    """Per source pixel: Jint = grad I1 . Jproj . JRt (:432-437, the true chain rule) and
    Jdep = gain * (grad D1 . Jproj . JRt - JRt[z,:]) (:440-448); gradients read at the SOURCE index (:424-431)."""
    with np.errstate(all="ignore"):
        JRt = _jacobian_rt(wp["px"], wp["py"], wp["pz"], state)
        iz, fx, fy = wp["iz"], wp["fx"], wp["fy"]
        n = iz.size
        Jp = np.zeros((n, 2, 3))
        Jp[:, 0, 0] = fx * iz
        Jp[:, 1, 1] = fy * iz
        Jp[:, 0, 2] = -(fx * wp["X"]) * iz * iz
        Jp[:, 1, 2] = -(fy * wp["Y"]) * iz * iz
        JpR = np.einsum("nij,njk->nik", Jp, JRt)
        Jint = gx.ravel()[:, None] * JpR[:, 0, :] + gy.ravel()[:, None] * JpR[:, 1, :]
        Jdep = gain * (dgx.ravel()[:, None] * JpR[:, 0, :] + dgy.ravel()[:, None] * JpR[:, 1, :] - JRt[:, 2, :])
    return Jint, Jdep


def literal_system(i0, d0, i1, d1, gx, gy, dgx, dgy, gain, level, K, state, min_depth=0.3, max_depth=5.0):
    """(a) The reference's loop, pixel by pixel in raster order, into dense r[2N] and J[2N x 6] (:603-609 zero them)."""
    h, w = i0.shape
    n = h * w
    wp = warp(d0, level, K, state, min_depth, max_depth)
    Jint, Jdep = jacobians(wp, gx, gy, dgx, dgy, gain, state)
    r = np.zeros(2 * n)
    J = np.zeros((2 * n, 6))
    I0, D0, I1, D1 = i0.ravel(), d0.ravel(), i1.ravel(), d1.ravel()
    for i in range(n):
        if not wp["contrib"][i]:
            continue
        t = int(wp["tgt"][i])
        J[i] = Jint[i]                                  # :422-428
        r[t] = I1[t] - I0[i]                            # :431
        J[2 * i] = Jdep[i]                              # :434-439
        r[2 * t] = gain * (D1[t] - D0[i])               # :442-443
    return r, J, int(wp["contrib"].sum())


def normal_equations(i0, d0, i1, d1, gx, gy, dgx, dgy, gain, level, K, state, min_depth=0.3, max_depth=5.0):
    """(b) H, g from the owner map and the row-resolution rule.  Returns (H, g, stats)."""
    h, w = i0.shape
    n = h * w
    wp = warp(d0, level, K, state, min_depth, max_depth)
    contrib, tgt = wp["contrib"], wp["tgt"]
    Jint, Jdep = jacobians(wp, gx, gy, dgx, dgy, gain, state)
    owner = np.full(n, -1, dtype=np.int64)
    src = np.nonzero(contrib)[0]
    np.maximum.at(owner, tgt[src], src)                 # last raster writer = largest source index
    m = np.arange(2 * n)
    half = m // 2
    even = (m % 2) == 0
    below = m < n
    mc = np.minimum(m, n - 1)
    # J of row m
    use_int = below & contrib[mc] & (m > 0)
    use_dep = ~use_int & even & contrib[half]
    J = np.zeros((2 * n, 6))
    J[use_int] = Jint[m[use_int]]
    J[use_dep] = Jdep[half[use_dep]]
    # r of row m: larger candidate wins, tie (m = 0) to depth
    c_int = np.where(below, owner[mc], -1)
    c_dep = np.where(even, owner[half], -1)
    dep_wins = (c_dep >= 0) & (c_dep >= c_int)
    int_wins = ~dep_wins & (c_int >= 0)
    I0, D0, I1, D1 = i0.ravel(), d0.ravel(), i1.ravel(), d1.ravel()
    r = np.zeros(2 * n)
    with np.errstate(all="ignore"):
        r[int_wins] = I1[m[int_wins]] - I0[c_int[int_wins]]
        r[dep_wins] = gain * (D1[half[dep_wins]] - D0[c_dep[dep_wins]])
        H = J.T @ J
        g = J.T @ r
    stats = dict(contributing=int(contrib.sum()),
                 intensity_won=int(int_wins.sum()),
                 depth_won_below_n=int((dep_wins & below & (m > 0)).sum()),
                 row0_tie=int(n > 0 and dep_wins[0] and c_int[0] == c_dep[0]),     # (a level of zero pixels has no row 0)
                 jdep_below_n=int((use_dep & below).sum()),
                 depth_rows_at_n=int((use_dep & ~below).sum()))
    return H, g, stats


def reference_step(H, g):
    """(J^T J).inverse() * g as the reference evaluates it (:629-630) on the reference build's matrix stand-in: LU with
    partial pivoting on a row-major copy, one forward and one backward substitution per column of the identity (the
    operations of inverse6 in oracle/phovo_oracle.c, in its order), then the product summed left to right.  A singular
    matrix gives inf / NaN, as there, not an exception."""
    n = 6
    lu = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    perm = list(range(n))
    f64 = np.float64
    lu = [[f64(v) for v in row] for row in lu]
    for k in range(n):
        piv, best = k, abs(lu[k][k])
        for r in range(k + 1, n):
            if abs(lu[r][k]) > best:
                best, piv = abs(lu[r][k]), r
        if piv != k:
            lu[k], lu[piv] = lu[piv], lu[k]
            perm[k], perm[piv] = perm[piv], perm[k]
        d = lu[k][k]
        for r in range(k + 1, n):
            lu[r][k] = lu[r][k] / d
            f = lu[r][k]
            for c in range(k + 1, n):
                lu[r][c] = lu[r][c] - f * lu[k][c]
    inv = [[f64(0.0)] * n for _ in range(n)]
    for col in range(n):
        y = [f64(0.0)] * n
        for r in range(n):
            s = f64(1.0 if perm[r] == col else 0.0)
            for c in range(r):
                s = s - lu[r][c] * y[c]
            y[r] = s
        for r in range(n - 1, -1, -1):
            s = y[r]
            for c in range(r + 1, n):
                s = s - lu[r][c] * inv[c][col]
            inv[r][col] = s / lu[r][r]
    step = np.zeros(n)
    for a in range(n):
        s = inv[a][0] * f64(g[0])
        for b in range(1, n):
            s = s + inv[a][b] * f64(g[b])
        step[a] = s
    return step


def optimize(cfg, K, src_planes, tgt_planes, init_state=None, min_depth=0.3, max_depth=5.0):
    """(c) Optimize() (:587-648).  src_planes = (intensity pyramid, depth pyramid), tgt_planes = target_planes(...).
    Returns (state, iterations per level, contributing pixels of each level's last iteration, flags, stats per
    iteration).  A level with max_num_iterations 0 reports 1 iteration, as the reference counts it.  flags: the
    PHOVO_PAIR_* bits the device reports (NONFINITE 1, RANK_DEFICIENT 4)."""
    i0p, d0p = src_planes
    state = np.zeros(6) if init_state is None else np.array(init_state, dtype=np.float64)
    nl = cfg.num_levels
    iters, valid, flags, trace = [0] * nl, [0] * nl, 0, []
    for level in range(nl - 1, -1, -1):
        max_it = cfg.max_num_iterations[level]
        if max_it <= 0:
            iters[level] = 1             # the loop body runs once and computes nothing (:594-628), the test stops it
            continue
        it = 0
        while True:
            H, g, st = normal_equations(i0p[level], d0p[level], tgt_planes["i1"][level], tgt_planes["d1"][level],
                                        tgt_planes["gx"][level], tgt_planes["gy"][level], tgt_planes["dgx"][level],
                                        tgt_planes["dgy"][level], tgt_planes["gain"][level], level, K, state,
                                        min_depth, max_depth)
            with np.errstate(all="ignore"):
                step = reference_step(H, g)
            state = state - cfg.lambda_optimization_step[level] * step      # :638-639
            it += 1
            valid[level] = st["contributing"]
            trace.append(dict(level=level, iteration=it, H=H, **st))
            if st["contributing"] < 6:
                flags |= 4
            finite = bool(np.all(np.isfinite(state)))
            if not finite:
                flags |= 1
            if it >= max_it:                                                 # TestTerminationCriteria
                break
            if np.linalg.norm(g) < cfg.min_gradient_norm[level]:
                break
            if not finite:
                break
        iters[level] = it
    return state, iters, valid, flags, trace


def align(cfg, K, gray0, depth0, gray1, depth1, init_state=None, min_depth=0.3, max_depth=5.0):
    """SetSourceFrame + SetTargetFrame + Optimize through the checker."""
    src = oracle.build_source_pyramids(gray0, depth0, cfg)
    tgt = target_planes(gray1, depth1, cfg, max_depth)
    return optimize(cfg, K, src, tgt, init_state, min_depth, max_depth)
