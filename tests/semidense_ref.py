"""CPU checker of the semi-dense inverse-compositional objective (PHOVO_OBJECTIVE_INVERSE_SEMIDENSE), in numpy.

TEST INFRASTRUCTURE ONLY.  The objective is objective 5 run on a source whose depth has been set to NaN wherever the pixel is
not selected, and that sentence is the checker: select() is the mask, optimize() hands inverse_ref.optimize the masked planes.
rows_loop is the same definition written the way the kernel works -- a list of selected pixels built once, then walked -- one
pixel at a time, for tiny images.  `rule` swaps in a wrong selection rule (the mutants of tests/test_semidense_cpu.py); the
default is the contract's."""
import numpy as np

import inverse_ref as ir
from inverse_ref import pose_bar  # noqa: F401

RULES = ("contract", "strict", "l1")


def select(planes, tau, min_depth=0.3, max_depth=5.0, rule="contract"):
    """The mask [H, W]: min_depth < D0 < max_depth and GX0^2 + GY0^2 >= tau^2, in fp64 on the planes as given; NaN fails
    either comparison.  rule `strict`: > for >=; `l1`: |GX0| + |GY0| >= tau."""
    d0, gx0, gy0 = planes[1], planes[2], planes[3]
    with np.errstate(all="ignore"):
        depth_ok = (min_depth < d0) & (d0 < max_depth)
        if rule == "contract":
            grad_ok = gx0 * gx0 + gy0 * gy0 >= tau * tau
        elif rule == "strict":
            grad_ok = gx0 * gx0 + gy0 * gy0 > tau * tau
        elif rule == "l1":
            grad_ok = np.abs(gx0) + np.abs(gy0) >= tau
        else:
            raise KeyError(rule)
    return depth_ok & grad_ok


def masked(planes, tau, min_depth=0.3, max_depth=5.0, rule="contract"):
    """(the planes with D0 NaN off the mask, the number of selected pixels)."""
    m = select(planes, tau, min_depth, max_depth, rule)
    i0, d0, gx0, gy0, i1 = planes
    return (i0, np.where(m, d0, np.nan), gx0, gy0, i1), int(m.sum())


def threshold_gap(planes, tau, min_depth=0.3, max_depth=5.0):
    """The smallest |g^2 - tau^2| / tau^2 over the depth-valid pixels with a finite gradient (inf for tau = 0 or none)."""
    if not tau > 0 or not np.isfinite(tau * tau):
        return np.inf
    d0, gx0, gy0 = planes[1], planes[2], planes[3]
    with np.errstate(all="ignore"):
        ok = (min_depth < d0) & (d0 < max_depth)
        g2 = (gx0 * gx0 + gy0 * gy0)[ok]
    g2 = g2[np.isfinite(g2)]
    return float(np.abs(g2 - tau * tau).min() / (tau * tau)) if g2.size else np.inf


def optimize(pyr, K, cfg, tau, init_pose=None, rule="contract"):
    """inverse_ref.optimize on planes whose D0 is NaN off the mask; tau[L] per level.  Returns its record with
    `selected[L]` added (0 for levels with max_num_iterations 0)."""
    lo, hi = cfg.get("min_depth", 0.3), cfg.get("max_depth", 5.0)
    mp, selected = [], []
    for L in range(cfg["num_levels"]):
        if cfg["max_iter"][L] <= 0 or pyr[L] is None:
            mp.append(pyr[L])
            selected.append(0)
            continue
        planes, n = masked(pyr[L], tau[L], lo, hi, rule)
        mp.append(planes)
        selected.append(n)
    ref = ir.optimize(mp, K, cfg, init_pose)
    ref["selected"] = selected
    return ref


def pixel_list(planes, tau, min_depth=0.3, max_depth=5.0):
    """The selected pixels as (col, row), in raster order, from a pixel-by-pixel scan."""
    _, d0, gx0, gy0, _ = planes
    H, W = d0.shape
    out = []
    for k in range(H * W):
        rr, cc = divmod(k, W)
        pz, gx, gy = d0[rr, cc], gx0[rr, cc], gy0[rr, cc]
        if not (min_depth < pz < max_depth):
            continue
        if not (gx * gx + gy * gy >= tau * tau):
            continue
        out.append((cc, rr))
    return out


def rows_loop(planes, level, K, R, t, tau, min_depth=0.3, max_depth=5.0):
    """(r[N], J[N, 6], rows[N] bool, the list) with the list walked record by record: warp, bounds test, four clamped
    taps, residual and source-side row of inverse_ref.rows_loop for the listed pixels alone."""
    i0, d0, gx0, gy0, i1 = planes
    H, W = i0.shape
    fx, fy, ox, oy = ir._intrinsics(level, K)
    n = H * W
    r, J, rows = np.zeros(n), np.zeros((n, 6)), np.zeros(n, dtype=bool)
    lst = pixel_list(planes, tau, min_depth, max_depth)
    for cc, rr in lst:
        k = rr * W + cc
        pz = d0[rr, cc]
        p = np.array([(cc - ox) * pz / fx, (rr - oy) * pz / fy, pz])
        P = R @ p + t
        u, v = P[0] * fx / P[2] + ox, P[1] * fy / P[2] + oy
        if not (u > -0.5 and u < W - 0.5 and v > -0.5 and v < H - 0.5):
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
    return r, J, rows, lst
