"""CPU checker of the photometric-geometric objective (PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC), in numpy.

TEST INFRASTRUCTURE ONLY.  planes = (i0, d0, i1, gx1, gy1, d1) of a level; d1 is the target's depth plane.  The photometric
rows are the bilinear-corrected rows of oracle/numpy_twin.py -- the vectorised form calls
numpy_twin.normal_equations_bilinear(corrected=True) for them, as tests/affine_ref.py does -- and the depth rows are written
here on the twin's geometry (the same expressions for the moved point, the warped position, the clamped taps and the
derivative of the projection):
    r_D = sigma (D1(u, v) - Z'),   J_D = sigma (dgx dU/dp + dgy dV/dp - dZ'/dp)
on every photometric row whose four D1 taps pass min_depth < d < max_depth (NaN fails) and, with a residual limit > 0, whose
|D1(u, v) - Z'| is at most that limit.  rows_loop is the same definition written out pixel by pixel, for tiny images, with
counters of the branches it took; optimize is the level loop (the twin's, numpy.linalg.solve) and records per accepted state
cond(H), how close ||g|| came to min_gradient_norm and how close any row came to the residual gate."""
import numpy as np

from oracle import numpy_twin as twin

PAIR_NONFINITE, PAIR_RANK_DEFICIENT = 1, 4


def _rotation(pose):
    x, y, z, yaw, pitch, roll = [float(v) for v in pose]
    sy, cy, sp, cp, sr, cr = np.sin(yaw), np.cos(yaw), np.sin(pitch), np.cos(pitch), np.sin(roll), np.cos(roll)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return R, (sy, cy, sp, cp, sr, cr)


def rows_vectorised(planes, level, K, pose, sigma, limit, min_depth=0.3, max_depth=5.0):
    """Returns dict(rI[N], JI[N,6], rows[N], rD[N], JD[N,6], drows[N], gate_margin, cell_margin); everything outside its rows
    is zero.
    gate_margin: the smallest | |D1(u,v) - Z'| - limit | / limit over the photometric rows whose taps pass (inf: gate off).
    cell_margin: the smallest distance, in pixels, of any row's u or v from an integer.  The bilinear samples are continuous
    there, but WHICH four taps are read (the tap gate) and the derivative of the depth interpolant are not: a warp that
    lands within rounding of a pixel centre -- a zero start pose does, on every pixel -- takes the left or the right cell by
    the last bit of u, here and on the device independently."""
    i0, d0, i1, gx1, gy1, d1 = planes
    pose = np.asarray(pose, dtype=np.float64)
    five = (i0, d0, i1, gx1, gy1)
    with np.errstate(all="ignore"):
        rI, JI = twin.normal_equations_bilinear(five, level, K, pose, min_depth, max_depth, corrected=True)
        # which pixels are rows: the twin's own gate and bounds test, read off a run on I0 = 0, I1 = 1 (tests/affine_ref.py)
        z, o = np.zeros_like(i0), np.ones_like(i0)
        probe, _ = twin.normal_equations_bilinear((z, d0, o, z, z), level, K, pose, min_depth, max_depth, corrected=True)
        rows = probe != 0.0
        # the twin's geometry once more, for what it does not return
        H_, W_ = i0.shape
        sf = 1.0 / 2 ** level
        fx, fy, ox, oy = K[0, 0] * sf, K[1, 1] * sf, K[0, 2] * sf, K[1, 2] * sf
        x, y, zt = pose[:3]
        R, (sy, cy, sp, cp, sr, cr) = _rotation(pose)
        cc, rr = np.meshgrid(np.arange(W_, dtype=np.float64), np.arange(H_, dtype=np.float64))
        pz = d0.reshape(-1)
        px = (cc.reshape(-1) - ox) * pz / fx
        py = (rr.reshape(-1) - oy) * pz / fy
        P = R @ np.stack([px, py, pz]) + np.array([[x], [y], [zt]])
        iz = 1.0 / P[2]
        tc, tr = P[0] * fx * iz + ox, P[1] * fy * iz + oy
        tc, tr = np.where(rows, tc, 0.0), np.where(rows, tr, 0.0)
        cell_margin = np.inf
        if rows.any():
            cell_margin = float(min(np.abs(tc - np.rint(tc))[rows].min(), np.abs(tr - np.rint(tr))[rows].min()))
        fc, fr = np.floor(tc), np.floor(tr)
        ax, ay = tc - fc, tr - fr
        c0, c1 = np.clip(fc, 0, W_ - 1).astype(np.int64), np.clip(fc + 1, 0, W_ - 1).astype(np.int64)
        r0, r1 = np.clip(fr, 0, H_ - 1).astype(np.int64), np.clip(fr + 1, 0, H_ - 1).astype(np.int64)
        p00, p01, p10, p11 = d1[r0, c0], d1[r0, c1], d1[r1, c0], d1[r1, c1]
        taps_ok = rows.copy()
        for t in (p00, p01, p10, p11):
            taps_ok &= (min_depth < t) & (t < max_depth)
        dsm = (1 - ay) * ((1 - ax) * p00 + ax * p01) + ay * ((1 - ax) * p10 + ax * p11)
        dgx = (1 - ay) * (p01 - p00) + ay * (p11 - p10)
        dgy = (1 - ax) * (p10 - p00) + ax * (p11 - p01)
        res = dsm - P[2]
        drows = taps_ok.copy()
        gate_margin = np.inf
        if limit > 0:
            drows &= np.abs(res) <= limit
            if taps_ok.any():
                gate_margin = float(np.min(np.abs(np.abs(res[taps_ok]) - limit)) / limit)
        Xr, Yr, Zr = P[0] - x, P[1] - y, P[2] - zt
        zero, one = np.zeros_like(Xr), np.ones_like(Xr)
        dP = [np.stack([one, zero, zero]), np.stack([zero, one, zero]), np.stack([zero, zero, one]),
              np.stack([-Yr, Xr, zero]),
              np.stack([cy * Zr, sy * Zr, -(cp * px + sp * sr * py + sp * cr * pz)]),
              np.stack([R[0, 2] * py - R[0, 1] * pz, R[1, 2] * py - R[1, 1] * pz, R[2, 2] * py - R[2, 1] * pz])]
        JD = np.zeros((pz.size, 6))
        for j in range(6):
            du = fx * dP[j][0] * iz - fx * P[0] * dP[j][2] * iz ** 2
            dv = fy * dP[j][1] * iz - fy * P[1] * dP[j][2] * iz ** 2
            JD[:, j] = sigma * (dgx * du + dgy * dv - dP[j][2])
        rD = sigma * res
    JD[~drows] = 0.0
    rD = np.where(drows, rD, 0.0)
    return dict(rI=rI, JI=JI, rows=rows, rD=rD, JD=JD, drows=drows, gate_margin=gate_margin, cell_margin=cell_margin)


COUNTERS = ("gate", "oob", "tap_low", "tap_high", "tap_nan", "residual_gate", "photo_only", "c-", "c+", "r-", "r+",
            "zero_dgx", "zero_dgy")


def rows_loop(planes, level, K, pose, sigma, limit, min_depth=0.3, max_depth=5.0):
    """The same rows, one source pixel at a time in raster order (tiny images).  Returns the dict of rows_vectorised plus
    `stats`, the number of pixels that took each branch: the source depth gate, out of bounds, a D1 tap at or below
    min_depth / at or above max_depth / NaN, a row the residual gate dropped, a photometric row without a depth row, each
    clamp band of the taps, and a derivative that is exactly 0 because clamping made both taps one pixel."""
    i0, d0, i1, gx1, gy1, d1 = planes
    H, W = i0.shape
    sf = 1.0 / 2 ** level
    fx, fy, ox, oy = K[0, 0] * sf, K[1, 1] * sf, K[0, 2] * sf, K[1, 2] * sf
    x, y, z = [float(v) for v in pose[:3]]
    R, (sy, cy, sp, cp, sr, cr) = _rotation(pose)
    n = H * W
    out = dict(rI=np.zeros(n), JI=np.zeros((n, 6)), rows=np.zeros(n, dtype=bool), rD=np.zeros(n), JD=np.zeros((n, 6)),
               drows=np.zeros(n, dtype=bool), gate_margin=np.inf, cell_margin=np.inf)
    stats = {k: 0 for k in COUNTERS}
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
        out["cell_margin"] = min(out["cell_margin"], abs(tc - np.rint(tc)), abs(tr - np.rint(tr)))
        fc, fr = np.floor(tc), np.floor(tr)
        ax, ay = tc - fc, tr - fr
        c0, c1 = int(min(max(fc, 0), W - 1)), int(min(max(fc + 1, 0), W - 1))
        r0, r1 = int(min(max(fr, 0), H - 1)), int(min(max(fr + 1, 0), H - 1))
        if fc < 0: stats["c-"] += 1
        if fc + 1 > W - 1: stats["c+"] += 1
        if fr < 0: stats["r-"] += 1
        if fr + 1 > H - 1: stats["r+"] += 1

        def smp(Pl):
            return (1 - ay) * ((1 - ax) * Pl[r0, c0] + ax * Pl[r0, c1]) + ay * ((1 - ax) * Pl[r1, c0] + ax * Pl[r1, c1])
        Xr, Yr, Zr = P[0] - x, P[1] - y, P[2] - z
        dP = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]),
              np.array([-Yr, Xr, 0.0]),
              np.array([cy * Zr, sy * Zr, -(cp * px + sp * sr * py + sp * cr * pz)]),
              np.array([R[0, 2] * py - R[0, 1] * pz, R[1, 2] * py - R[1, 1] * pz, R[2, 2] * py - R[2, 1] * pz])]
        du = [fx * dP[j][0] * iz - fx * P[0] * dP[j][2] * iz ** 2 for j in range(6)]
        dv = [fy * dP[j][1] * iz - fy * P[1] * dP[j][2] * iz ** 2 for j in range(6)]
        gxs, gys = smp(gx1), smp(gy1)
        for j in range(6):
            out["JI"][k, j] = gxs * du[j] + gys * dv[j]
        out["rI"][k] = smp(i1) - i0[rr, cc]
        out["rows"][k] = True
        # the depth row
        taps = [d1[r0, c0], d1[r0, c1], d1[r1, c0], d1[r1, c1]]
        ok = True
        for t in taps:
            if np.isnan(t):
                stats["tap_nan"] += 1; ok = False
            elif not (min_depth < t):
                stats["tap_low"] += 1; ok = False
            elif not (t < max_depth):
                stats["tap_high"] += 1; ok = False
        if not ok:
            stats["photo_only"] += 1
            continue
        p00, p01, p10, p11 = taps
        res = smp(d1) - P[2]
        if limit > 0:
            out["gate_margin"] = min(out["gate_margin"], abs(abs(res) - limit) / limit)
            if not (abs(res) <= limit):
                stats["residual_gate"] += 1
                stats["photo_only"] += 1
                continue
        dgx = (1 - ay) * (p01 - p00) + ay * (p11 - p10)
        dgy = (1 - ax) * (p10 - p00) + ax * (p11 - p01)
        if c0 == c1:
            assert dgx == 0.0
            stats["zero_dgx"] += 1
        if r0 == r1:
            assert dgy == 0.0
            stats["zero_dgy"] += 1
        for j in range(6):
            out["JD"][k, j] = sigma * (dgx * du[j] + dgy * dv[j] - dP[j][2])
        out["rD"][k] = sigma * res
        out["drows"][k] = True
    out["stats"] = stats
    return out


def system(planes, level, K, pose, sigma, limit, min_depth=0.3, max_depth=5.0):
    """dict(g[6], H[6,6], rows, depth_rows, photometric_cost, depth_cost, gate_margin, cell_margin) at the pose."""
    v = rows_vectorised(planes, level, K, pose, sigma, limit, min_depth, max_depth)
    with np.errstate(all="ignore"):
        g = v["JI"].T @ v["rI"] + v["JD"].T @ v["rD"]
        Hm = v["JI"].T @ v["JI"] + v["JD"].T @ v["JD"]
        ci, cd = float(v["rI"] @ v["rI"]), float(v["rD"] @ v["rD"])
    return dict(g=g, H=Hm, rows=int(v["rows"].sum()), depth_rows=int(v["drows"].sum()), photometric_cost=ci,
                depth_cost=cd, gate_margin=v["gate_margin"], cell_margin=v["cell_margin"])


def optimize(pyr, K, cfg, init_pose=None):
    """pyr[L] = (i0, d0, i1, gx1, gy1, d1); cfg: dict(num_levels, lam, max_iter, min_grad, depth_weight,
    max_depth_residual[, min_depth, max_depth]).  The bilinear extension's level loop: per iteration x <- x - lambda_L H^-1 g,
    the level ends when the iteration count is reached or ||g||_2 < min_gradient_norm[L], tested after the step; a state that
    is not finite ends the level too.  Levels with max_num_iterations 0 are skipped (they report one iteration).
    Returns dict(state[6], iterations[L], valid_pixels[L], depth_rows[L], photometric_cost[L], depth_cost[L], flags,
    gradient_norm, cond, margin, h_norm, noise_level, gate_margin) -- cond, margin, h_norm and noise_level as in
    tests/affine_ref.py (noise_level: the first level with an iteration of 1 ... 5 photometric rows); gate_margin: the smallest
    | |D1(u,v) - Z'| - max_depth_residual | / max_depth_residual over all rows of all accepted states (inf: gate off);
    cell_margin: the smallest distance (pixels) of any row's u or v from an integer over all those states (rows_vectorised)."""
    nl = cfg["num_levels"]
    state = np.zeros(6) if init_pose is None else np.array(init_pose, dtype=np.float64)
    iters, valid, drows, cost_i, cost_d = [0] * nl, [0] * nl, [0] * nl, [0.0] * nl, [0.0] * nl
    flags, gnorm, cond, margin, h_norm, noise_level, gate_margin = 0, 0.0, 0.0, np.inf, 0.0, None, np.inf
    cell_margin = np.inf
    for L in range(nl - 1, -1, -1):
        if cfg["max_iter"][L] <= 0:
            iters[L] = 1
            continue
        it = 0
        while True:
            s = system(pyr[L], L, K, state, cfg["depth_weight"][L], cfg["max_depth_residual"][L],
                       cfg.get("min_depth", 0.3), cfg.get("max_depth", 5.0))
            g, Hm = s["g"], s["H"]
            valid[L], drows[L], cost_i[L], cost_d[L] = s["rows"], s["depth_rows"], s["photometric_cost"], s["depth_cost"]
            gate_margin = min(gate_margin, s["gate_margin"])
            cell_margin = min(cell_margin, s["cell_margin"])
            if s["rows"] < 6:
                flags |= PAIR_RANK_DEFICIENT
                if s["rows"] > 0 and noise_level is None:
                    noise_level = L
            try:
                with np.errstate(all="ignore"):
                    step = np.linalg.solve(Hm, g)
                    cond = max(cond, float(np.linalg.cond(Hm)))
            except np.linalg.LinAlgError:                       # an exactly singular system: the device's 1 / 0
                step = np.full(6, np.nan)
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
    return dict(state=state, iterations=iters, valid_pixels=valid, depth_rows=drows, photometric_cost=cost_i,
                depth_cost=cost_d, flags=flags, gradient_norm=gnorm, cond=cond, margin=margin, h_norm=h_norm,
                noise_level=noise_level, gate_margin=gate_margin, cell_margin=cell_margin)


def pose_bar(cond, states, flat=1e-9):
    """affine_ref.pose_bar: the project's parity bar flat x max(1, |x|), widened where cond(H) exceeds 1e5 (capped at 1e-5)."""
    return min(1e-5, flat * max(1.0, cond / 1e5)) * max(1.0, float(np.abs(states).max()))
