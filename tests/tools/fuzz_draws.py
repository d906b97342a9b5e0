"""Draws and measures shared by the randomised sweeps (fuzz_parity.py, fuzz_objectives.py).  Pure numpy: no GPU."""
import numpy as np


def worst_condition(trace):
    c = 1.0
    for e in trace:
        h = e["hessian"]
        if np.all(np.isfinite(h)) and np.any(h != 0.0):
            c = max(c, float(np.linalg.cond(h)))
    return c


P4 = 0.78539816339744828          # fl(pi/4): beyond it the device takes the library's sincos


def draw_angle(rs, axis, truth):
    """One Euler angle of an initial state (axis 0 = yaw): every branch of the device's sin / cos and both thresholds."""
    kind, sign, u = int(rs.randint(0, 7)), float(rs.choice([-1.0, 1.0])), rs.rand()
    if kind == 0:
        return truth + 0.05 * (u - 0.5)                                   # near the truth (for yaw: up to 0.9 rad)
    if kind == 1:
        return sign * 0.3 * u                                             # branch 1
    if kind == 2:
        return sign * (0.3 + (P4 - 0.3) * u)                              # branch 2
    if kind == 3:                                                         # within 3 ulp of 0.3, 0.78125, fl(pi/4)
        a, steps = float(rs.choice([0.3, 0.78125, P4])), int(rs.randint(-3, 4))
        for _ in range(abs(steps)):
            a = float(np.nextafter(a, np.inf if steps > 0 else -np.inf))
        return sign * a
    if kind == 4:
        return sign * (P4 + 0.5 * u)                                      # branch 3, just beyond
    if kind == 5 and axis > 0:
        return sign * (np.pi - 0.2 - 0.3 * u)                             # pitch / roll beyond pi/2: behind the camera
    return sign * 0.01 * u


def reference_sweep_case(index):
    """Draw `index` of the sweep that holds the oracle (CPU) and the HIP path (GPU) to the reference build
    (tests/test_reference_build_cpu.py, tests/test_gpu_reference_parity.py): one seed per draw, so both tests see the
    same cases.  Sizes 24x20 ... 200x150 on 1-3 levels, intrinsics off the half-integers, holes / NaN / out-of-range
    depth, 0-6 iterations per level with fixed counts or gradient thresholds, damped steps, and initial states from
    none, small, or an Euler angle from each branch of the device's sin / cos (draw_angle).  Returns the arguments
    of synthetic.make_pair and everything drawn after it; the caller renders the pair."""
    rs = np.random.RandomState(770000 + index)
    nl = int(rs.randint(1, 4))
    unit = 2 ** (nl - 1)
    w = max(int(rs.randint(24, 201)) // unit * unit, 8 * unit)
    h = max(int(rs.randint(20, 151)) // unit * unit, 8 * unit)
    pair = dict(seed=9000 + index, width=w, height=h, holes=float(rs.choice([0.0, 0.02, 0.2])),
                trans=float(rs.choice([0.002, 0.02, 0.08])), rot=float(rs.choice([0.001, 0.01, 0.05])))
    k_shift = None
    if rs.rand() < 0.6:
        k_shift = (rs.uniform(-3, 3), rs.uniform(-3, 3), rs.uniform(0.9, 1.1), rs.uniform(0.9, 1.1))
    contaminate = int(rs.randint(0, 2 ** 31 - 1)) if rs.rand() < 0.3 else None
    max_iter = [int(rs.randint(0, 7)) for _ in range(nl)]
    if sum(max_iter) == 0:
        max_iter[-1] = 3
    fixed = rs.rand() < 0.5
    min_grad = [0.0] * nl if fixed else [float(rs.choice([1.0, 30.0, 300.0])) for _ in range(nl)]
    lam = [float(rs.choice([1.0, 0.7])) for _ in range(nl)]
    kind = rs.rand()
    init = None
    if kind >= 0.4:
        init = rs.uniform(-1, 1, 6) * np.array([0.02, 0.02, 0.02, 0.01, 0.01, 0.01])
    if kind >= 0.8:
        init[3 + int(rs.randint(0, 3))] = draw_angle(rs, 0, 0.0)        # axis 0: never the behind-the-camera kind
    return dict(pair=pair, k_shift=k_shift, contaminate=contaminate, num_levels=nl, max_iter=max_iter,
                min_grad=min_grad, lam=lam, init=init)


def reference_sweep_inputs(case, make_pair):
    """Render a draw of reference_sweep_case: (K, gray0, depth0, gray1, depth1)."""
    p = make_pair(**case["pair"])
    K = p["K"].copy()
    if case["k_shift"] is not None:
        dx, dy, sx, sy = case["k_shift"]
        K[0, 2] += dx
        K[1, 2] += dy
        K[0, 0] *= sx
        K[1, 1] *= sy
    d0 = p["depth0"].copy()
    if case["contaminate"] is not None:
        rs = np.random.RandomState(case["contaminate"])
        h, w = d0.shape
        d0[rs.rand(h, w) < 0.01] = np.nan
        d0[rs.rand(h, w) < 0.01] = 7.5      # beyond max depth
        d0[rs.rand(h, w) < 0.01] = -1.0
    return K, p["gray0"], d0, p["gray1"], p["depth1"]
