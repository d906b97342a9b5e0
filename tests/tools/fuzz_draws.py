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
