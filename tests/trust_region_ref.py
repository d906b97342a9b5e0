"""CPU checker of the trust-region (Levenberg-Marquardt) aligner, phovo::Ceres::CPhotoconsistencyOdometryCeres
(phovo/include/CPhotoconsistencyOdometryCeres.h, "Ceres.h" below; third_party/sample.h).  Test infrastructure, not
collected as tests.

It restates the contract of DESIGN.md §12 on top of the oracle's pyramid functions:
  (a) literal_rows    the per-pixel loop of ResidualRGBDPhotoconsistency::operator() (Ceres.h:157-269) over a dense
                      N-vector, with a small forward-mode dual number standing in for the Jet; for tiny images;
  (b) evaluate        the same rows, vectorised through the owner map (the largest source index landing on a target owns
                      its residual and its row), with the device's operation order (no fused multiply-adds);
  (c) optimize_level  the Levenberg-Marquardt loop of DESIGN.md §12 (our reading of Ceres 1.14's TrustRegionMinimizer),
                      taking the model cost change from the N-vector as Ceres does, recording every decision and its
                      margin.
"""
import math

import numpy as np

from oracle import oracle

DBL_MAX = np.finfo(np.float64).max
NOISE = 1e-10          # relative size of a cost change below which a decision on it is decided by rounding
(TR_SKIPPED, TR_MAX_ITERATIONS, TR_GRADIENT, TR_FUNCTION, TR_PARAMETER, TR_MIN_RADIUS, TR_INVALID_STEP,
 TR_EVALUATION_FAILED) = range(8)


def level_intrinsics(K, level):
    """Ceres.h:164-169: divisions by 2^L, then the inverses."""
    s = 2.0 ** level
    fx, fy, ox, oy = K[0][0] / s, K[1][1] / s, K[0][2] / s, K[1][2] / s
    return fx, fy, ox, oy, 1.0 / fx, 1.0 / fy


def _sin(a):
    return math.sin(a) if math.isfinite(a) else math.nan          # (math.sin raises on inf; the device gives NaN)


def _cos(a):
    return math.cos(a) if math.isfinite(a) else math.nan


def rotation(state):
    """Rt of Ceres.h:179-202 (eigenPose's matrix), with the device's association."""
    x, y, z, yaw, pitch, roll = [float(v) for v in state]
    sy, cy, sp, cp, sr, cr = _sin(yaw), _cos(yaw), _sin(pitch), _cos(pitch), _sin(roll), _cos(roll)
    R = np.array([[cp * cy, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [cp * sy, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return R, np.array([x, y, z]), (sy, cy, sp, cp, sr, cr)


# ---- (a) the literal loop with dual numbers ---------------------------------------------------------------------
class Dual:
    """value + 6 derivatives: what a ceres::Jet<double, 6> carries."""
    __slots__ = ("a", "v")

    def __init__(self, a, v=None):
        self.a = float(a)
        self.v = np.zeros(6) if v is None else v

    @staticmethod
    def _c(o):
        return o if isinstance(o, Dual) else Dual(o)

    def __add__(self, o):
        o = Dual._c(o)
        return Dual(self.a + o.a, self.v + o.v)

    __radd__ = __add__

    def __sub__(self, o):
        o = Dual._c(o)
        return Dual(self.a - o.a, self.v - o.v)

    def __rsub__(self, o):
        return Dual._c(o) - self

    def __mul__(self, o):
        o = Dual._c(o)
        return Dual(self.a * o.a, self.a * o.v + o.a * self.v)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual._c(o)
        q = self.a / o.a
        return Dual(q, (self.v - q * o.v) / o.a)

    def __rtruediv__(self, o):
        return Dual._c(o) / self

    def __neg__(self):
        return Dual(-self.a, -self.v)


def dsin(d):
    return Dual(math.sin(d.a), math.cos(d.a) * d.v)


def dcos(d):
    return Dual(math.cos(d.a), -math.sin(d.a) * d.v)


def linear_axis(c, size):
    """LinearInitAxis after SampleLinear's -0.5 shift (sample.h:32-51, 66-67): (tap0, tap1, weight of tap0)."""
    a = c - 0.5
    i = int(a)                                   # truncation toward zero
    if i < 0:
        return 0, 0, 1.0                         # (unreachable: a >= -0.5)
    if i > size - 2:
        return size - 1, size - 1, 1.0
    return i, i + 1, (i + 1) - a


def sample_linear(img, u, v):
    h, w = img.shape
    x1, x2, wx = linear_axis(u, w)
    y1, y2, wy = linear_axis(v, h)
    return (wy * (wx * img[y1, x1] + (1.0 - wx) * img[y1, x2]) +
            (1.0 - wy) * (wx * img[y2, x1] + (1.0 - wx) * img[y2, x2]))


def literal_rows(i0, d0, i1, gx, gy, level, K, state, min_depth=0.3, max_depth=5.0):
    """(a) residuals r[N] and Jacobian J[N x 6] as the reference's operator() writes them, pixel by pixel in raster order
    (later writers overwrite), with Dual numbers for the state."""
    h, w = i0.shape
    n = h * w
    fx, fy, ox, oy, ifx, ify = level_intrinsics(K, level)
    s = [Dual(float(state[k]), np.eye(6)[k].copy()) for k in range(6)]
    x, y, z, yaw, pitch, roll = s
    syw, cyw, sp, cp, sr, cr = dsin(yaw), dcos(yaw), dsin(pitch), dcos(pitch), dsin(roll), dcos(roll)
    Rt = [[cyw * cp, cyw * sp * sr - syw * cr, cyw * sp * cr + syw * sr, x],
          [syw * cp, syw * sp * sr + cyw * cr, syw * sp * cr - cyw * sr, y],
          [-sp, cp * sr, cp * cr, z]]
    r = np.zeros(n)
    J = np.zeros((n, 6))
    owner = np.full(n, -1)
    for row in range(h):
        for col in range(w):
            d = float(d0[row, col])
            if not (min_depth < d < max_depth):
                continue
            p = [(col - ox) * d * ifx, (row - oy) * d * ify, d]
            q = [Rt[k][0] * p[0] + Rt[k][1] * p[1] + Rt[k][2] * p[2] + Rt[k][3] for k in range(3)]
            tc = (q[0] * fx) / q[2] + ox
            tr = (q[1] * fy) / q[2] + oy
            if not (tr.a >= 0.0 and tr.a < h and tc.a >= 0.0 and tc.a < w):
                continue
            t = w * int(tr.a) + int(tc.a)
            val = sample_linear(i1, tc.a, tr.a)
            sgx, sgy = sample_linear(gx, tc.a, tr.a), sample_linear(gy, tc.a, tr.a)
            r[t] = val - i0[row, col]
            J[t] = sgx * tc.v + sgy * tr.v                    # ceres::Chain::Rule(sample, gradient, (x, y))
            owner[t] = row * w + col
    return r, J, int((owner >= 0).sum())


# ---- (b) vectorised rows through the owner map ---------------------------------------------------------------------
def _bilinear_vec(img, u, v):
    h, w = img.shape
    a = u - 0.5
    i = np.trunc(a).astype(np.int64)
    clampx = i > w - 2
    x1 = np.where(clampx, w - 1, i)
    x2 = np.where(clampx, w - 1, i + 1)
    wx = np.where(clampx, 1.0, (i + 1).astype(np.float64) - a)
    b = v - 0.5
    j = np.trunc(b).astype(np.int64)
    clampy = j > h - 2
    y1 = np.where(clampy, h - 1, j)
    y2 = np.where(clampy, h - 1, j + 1)
    wy = np.where(clampy, 1.0, (j + 1).astype(np.float64) - b)
    f = img.ravel()
    k11, k12, k21, k22 = y1 * w + x1, y1 * w + x2, y2 * w + x1, y2 * w + x2
    return wy * (wx * f[k11] + (1.0 - wx) * f[k12]) + (1.0 - wy) * (wx * f[k21] + (1.0 - wx) * f[k22])


def evaluate(i0, d0, i1, gx, gy, level, K, state, min_depth=0.3, max_depth=5.0):
    """(b) the N-vector r, J[N x 6] and cost, g, H, rows at `state`, in the device kernel's operation order."""
    h, w = i0.shape
    n = h * w
    fx, fy, ox, oy, ifx, ify = level_intrinsics(K, level)
    R, tv, (sy, cy, sp, cp, sr, cr) = rotation(state)
    k = np.arange(n)
    rd = (k // w).astype(np.float64)
    cd = (k % w).astype(np.float64)
    d = d0.ravel().astype(np.float64)
    with np.errstate(all="ignore"):
        px = (cd - ox) * d * ifx
        py = (rd - oy) * d * ify
        pz = d
        a0 = R[0, 0] * px + R[0, 1] * py + R[0, 2] * pz
        a1 = R[1, 0] * px + R[1, 1] * py + R[1, 2] * pz
        a2 = R[2, 0] * px + R[2, 1] * py + R[2, 2] * pz
        q0, q1, q2 = a0 + tv[0], a1 + tv[1], a2 + tv[2]
        u = (q0 * fx) / q2 + ox
        v = (q1 * fy) / q2 + oy
        ok = (min_depth < d) & (d < max_depth) & (v >= 0.0) & (v < h) & (u >= 0.0) & (u < w)
    src = np.nonzero(ok)[0]
    tgt = w * np.trunc(v[src]).astype(np.int64) + np.trunc(u[src]).astype(np.int64)
    owner = np.full(n, -1, dtype=np.int64)
    np.maximum.at(owner, tgt, src)
    own = owner[tgt] == src
    s, t = src[own], tgt[own]
    us, vs = u[s], v[s]
    with np.errstate(all="ignore"):
        I1s = _bilinear_vec(i1, us, vs)
        GXs = _bilinear_vec(gx, us, vs)
        GYs = _bilinear_vec(gy, us, vs)
        res = I1s - i0.ravel()[s]
        iz = 1.0 / q2[s]
        du0, dv1 = fx * iz, fy * iz
        du2, dv2 = -fx * q0[s] * iz * iz, -fy * q1[s] * iz * iz
        ju, jv, jw = GXs * du0, GYs * dv1, GXs * du2 + GYs * dv2
        spsr, spcr = sp * sr, sp * cr
        dq2_pitch = -(cp * px[s] + spsr * py[s] + spcr * pz[s])
        dq0_roll = R[0, 2] * py[s] - R[0, 1] * pz[s]
        dq1_roll = R[1, 2] * py[s] - R[1, 1] * pz[s]
        dq2_roll = R[2, 2] * py[s] - R[2, 1] * pz[s]
        Jrows = np.stack([ju, jv, jw, jv * a0[s] - ju * a1[s], (ju * cy + jv * sy) * a2[s] + jw * dq2_pitch,
                          ju * dq0_roll + jv * dq1_roll + jw * dq2_roll], -1)
    r = np.zeros(n)
    J = np.zeros((n, 6))
    r[t] = res
    J[t] = Jrows
    return system(r, J, rows=int(s.size)) | dict(owner=owner, u=u, v=v, ok=ok)


def system(r, J, rows=None):
    """cost, g, H of an N-vector of residuals and its Jacobian, and whether they are finite."""
    with np.errstate(all="ignore"):
        cost = 0.5 * float(r @ r)
        g = J.T @ r
        H = J.T @ J
    finite = bool(np.isfinite(cost) and np.all(np.isfinite(g)) and np.all(np.isfinite(H)))
    return dict(r=r, J=J, cost=cost, g=g, H=H, rows=int(np.count_nonzero(np.any(J != 0, 1))) if rows is None else rows,
                finite=finite)


# ---- (c) the Levenberg-Marquardt loop --------------------------------------------------------------------------------
def _margin(a, b):
    """Relative distance of a decision value from its threshold (1 when the threshold is 0 and the value is not)."""
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    den = max(abs(a), abs(b))
    return abs(a - b) / den if np.isfinite(den) else 1.0


def _cond(ev):
    """Condition number of an evaluation's J^T J (1 where it is zero or not finite; inf where it is singular)."""
    H = ev["H"]
    if not (np.all(np.isfinite(H)) and np.any(H != 0.0)):
        return 1.0
    return float(np.linalg.cond(H))


def optimize_level(evaluate_at, x0, max_iterations, function_tolerance, gradient_tolerance, parameter_tolerance,
                   initial_radius, max_radius, min_radius, min_relative_decrease):
    """(c) One level.  evaluate_at(x) returns a dict of `system`.  Returns (x, record) with record
    = dict(steps, accepted, termination, rows, initial_cost, final_cost, final_radius, g, decisions, margins)."""
    x = np.array(x0, dtype=np.float64)
    ev = evaluate_at(x)
    rec = dict(steps=0, accepted=0, termination=None, rows=ev["rows"], initial_cost=ev["cost"], final_cost=ev["cost"],
               final_radius=initial_radius, g=ev["g"], S=np.zeros(6), decisions=[], margins=[], min_rel_dc=np.inf,
               noise_from=None, accepted_before_noise=0, x0=x.copy(), g0=ev["g"], H=ev["H"], cond=_cond(ev))
    if not (np.isfinite(ev["cost"]) and ev["finite"]):
        rec["termination"] = TR_EVALUATION_FAILED
        return x, rec
    cur = ev
    S = 1.0 / (1.0 + np.sqrt(np.diag(cur["H"])))
    rec["S"] = S
    radius, decrease, ok, it = float(initial_radius), 2.0, True, 0

    def note(kind, value, threshold):
        if rec["noise_from"] is None:             # (decisions after the noise floor carry no margin: see below)
            rec["decisions"].append((kind, float(value), float(threshold)))
            rec["margins"].append(_margin(value, threshold))

    while True:
        if it >= max_iterations:
            term = TR_MAX_ITERATIONS
            break
        # (fmax skips a NaN coordinate of x, as the device's fmax does: a NaN initial state meets a zero gradient here)
        with np.errstate(invalid="ignore"):
            gmax = float(np.fmax.reduce(np.abs(x - (x - cur["g"])), initial=0.0))
        if ok:
            note("gradient", gmax, gradient_tolerance)
            if gmax <= gradient_tolerance:
                term = TR_GRADIENT
                break
        if radius <= min_radius:
            term = TR_MIN_RADIUS
            break
        it += 1
        Js = cur["J"] * S
        Hs = S[:, None] * cur["H"] * S[None, :]
        gs = S * cur["g"]
        A = Hs + np.diag(np.clip(np.diag(Hs), 1e-6, 1e32) / radius)
        try:
            L = np.linalg.cholesky(A)
            y = np.linalg.solve(L.T, np.linalg.solve(L, gs))
            solved = True
        except np.linalg.LinAlgError:
            y, solved = np.full(6, np.nan), False
        step = -y
        with np.errstate(all="ignore"):
            mr = Js @ step
            mcc = -float(mr @ (cur["r"] + 0.5 * mr))
        note("mcc", mcc, 0.0)
        if not solved or not np.all(np.isfinite(step)) or not (mcc > 0):
            term = TR_INVALID_STEP
            break
        cand = x + S * step
        step_norm = float(np.linalg.norm(x - cand))
        bound = parameter_tolerance * (float(np.linalg.norm(x)) + parameter_tolerance)
        note("parameter", step_norm, bound)
        if step_norm <= bound:
            term = TR_PARAMETER
            break
        cev = evaluate_at(cand)
        cand_cost = cev["cost"] if np.isfinite(cev["cost"]) else DBL_MAX
        dc = cur["cost"] - cand_cost
        # The noise floor: the function test and the acceptance test compare the cost change dc with thresholds, and two
        # implementations that sum the cost in different orders agree on dc only to ~1e-13 of the cost.  Once a decision
        # lies within NOISE x cost of its threshold it is decided by rounding (a level run with zero tolerances gets there
        # when it has converged), and so is everything after it: from that step on the record is not comparable decision
        # by decision.
        if rec["noise_from"] is None and cand_cost != DBL_MAX and (
                abs(abs(dc) - function_tolerance * cur["cost"]) <= NOISE * cur["cost"] or
                abs(dc - min_relative_decrease * mcc) <= NOISE * cur["cost"]):
            rec["noise_from"] = it
            rec["accepted_before_noise"] = rec["accepted"]
        note("function", abs(dc), function_tolerance * cur["cost"])
        if abs(dc) <= function_tolerance * cur["cost"]:
            term = TR_FUNCTION
            break
        rho = -DBL_MAX if cand_cost == DBL_MAX else dc / mcc
        note("rho", rho, min_relative_decrease)
        if rho > min_relative_decrease:
            # (how well rho -- and with it the radius update -- is conditioned: its rounding is ~eps * cost / |dc|)
            rec["min_rel_dc"] = min(rec["min_rel_dc"], abs(dc) / cur["cost"] if cur["cost"] > 0 else np.inf)
            x = cand
            cur = cev
            rec["accepted"] += 1
            rec["cond"] = max(rec["cond"], _cond(cev))
            if not cev["finite"]:
                term = TR_EVALUATION_FAILED
                break
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease, ok = 2.0, True
        else:
            radius /= decrease
            decrease *= 2.0
            ok = False
    rec.update(steps=it, termination=term, rows=cur["rows"], final_cost=cur["cost"], final_radius=radius, g=cur["g"], H=cur["H"])
    return x, rec


def pair_flags(x, records):
    """The PHOVO_PAIR_* bits of a pair's report after optimize(): NONFINITE (1) when an evaluation failed or the state is
    not finite, RANK_DEFICIENT (4) when a level ended with fewer than 6 rows."""
    flags = 0
    if not np.all(np.isfinite(x)) or any(r["termination"] == TR_EVALUATION_FAILED for r in records.values()):
        flags |= 1
    if any(r["rows"] < 6 for r in records.values()):
        flags |= 4
    return flags


def level_options(opt, level):
    """The solver options of one level from a native.TrustRegionOptions (or anything with the same per-level fields)."""
    return dict(function_tolerance=opt.function_tolerance[level], gradient_tolerance=opt.gradient_tolerance[level],
                parameter_tolerance=opt.parameter_tolerance[level],
                initial_radius=opt.initial_trust_region_radius[level], max_radius=opt.max_trust_region_radius[level],
                min_radius=opt.min_trust_region_radius[level], min_relative_decrease=opt.min_relative_decrease[level])


def optimize(cfg, K, src, tgt, opt, init_state=None, min_depth=0.3, max_depth=5.0):
    """Optimize() (Ceres.h:433-500): levels coarse to fine, those with max_num_iterations 0 skipped, the state handed on.
    src = (intensity pyramid, depth pyramid), tgt = (intensity, grad x, grad y pyramids); cfg: an oracle or native Config.
    Returns (state, {level: record})."""
    i0p, d0p = src
    i1p, gxp, gyp = tgt
    x = np.zeros(6) if init_state is None else np.array(init_state, dtype=np.float64)
    records = {}
    for level in range(cfg.num_levels - 1, -1, -1):
        mi = int(cfg.max_num_iterations[level])
        if mi <= 0:
            continue
        x, records[level] = optimize_level(
            lambda s, L=level: evaluate(i0p[L], d0p[L], i1p[L], gxp[L], gyp[L], L, K, s, min_depth, max_depth),
            x, mi, **level_options(opt, level))
    return x, records


def align(cfg, K, gray0, depth0, gray1, opt, init_state=None, min_depth=0.3, max_depth=5.0):
    """SetSourceFrame + SetTargetFrame + Optimize through the checker (cfg: an oracle Config)."""
    src = oracle.build_source_pyramids(gray0, depth0, cfg)
    tgt = oracle.build_target_pyramids(gray1, cfg)
    return optimize(cfg, K, src, tgt, opt, init_state, min_depth, max_depth)


def oracle_config(cfg):
    """An oracle Config with the levels, blur, gradient scales and iterations of a native Config."""
    nl = cfg.num_levels
    return oracle.make_config(num_levels=nl, blur=list(cfg.blur_filter_size[:nl]),
                              grad_scale=list(cfg.image_gradients_scaling_factor[:nl]),
                              max_iter=list(cfg.max_num_iterations[:nl]))
