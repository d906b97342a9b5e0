"""States at the edges of the device's sin / cos (write_pose_constants, gn_device.hpp), shared by the CPU checks of the
checkers' derivatives and the GPU tests of every kernel form.  Test infrastructure, not collected as tests."""
import numpy as np
import pytest

BASE = (0.01, -0.02, 0.015, 0.002, -0.001, 0.003)
ANGLES = (0.31, 0.55, 0.783, 0.80, 1.2)          # branch 2 (up to fl(pi/4)) and branch 3 (the library's sincos)


def initial_states():
    """Per axis a handful of angles from each branch, both signs; pitch and roll at pi - 0.3 (the scene behind the camera)."""
    out = []
    for axis in range(3):
        for a in ANGLES:
            for sg in (1.0, -1.0):
                s = np.array(BASE)
                s[3 + axis] = sg * a
                out.append(s)
    for axis in (1, 2):
        s = np.array(BASE)
        s[3 + axis] = np.pi - 0.3
        out.append(s)
    return out


# true in-plane motions (yaw) of 0.5, 0.7 and 0.9 rad: branches 2, 2, 3
MOTIONS = [[0.01, -0.005, 0.004, yaw, 0.002, -0.003] for yaw in (0.5, 0.7, 0.9)]
NEAR = np.array([0.004, 0.002, -0.003, 0.01, -0.004, 0.003])           # a start near the truth


def chain_rule_model():
    """du/dx, dv/dx and dZ/dx (x = the state) of the projection u, v = fx X / Z + ox, fy Y / Z + oy of q = Rt(x) p, in
    sympy: a callable of (x, y, z, yaw, pitch, roll, px, py, pz, fx, fy, ox, oy) returning 18 values."""
    sympy = pytest.importorskip("sympy")
    x, y, z, yaw, pitch, roll, px, py, pz, fx, fy, ox, oy = sympy.symbols(
        "x y z yaw pitch roll px py pz fx fy ox oy", real=True)
    c, s = sympy.cos, sympy.sin
    Rt = sympy.Matrix([
        [c(yaw) * c(pitch), c(yaw) * s(pitch) * s(roll) - s(yaw) * c(roll), c(yaw) * s(pitch) * c(roll) + s(yaw) * s(roll), x],
        [s(yaw) * c(pitch), s(yaw) * s(pitch) * s(roll) + c(yaw) * c(roll), s(yaw) * s(pitch) * c(roll) - c(yaw) * s(roll), y],
        [-s(pitch), c(pitch) * s(roll), c(pitch) * c(roll), z],
        [0, 0, 0, 1]])
    P = Rt * sympy.Matrix([px, py, pz, 1])
    u = P[0] * fx / P[2] + ox
    v = P[1] * fy / P[2] + oy
    params = (x, y, z, yaw, pitch, roll)
    out = [sympy.diff(u, p) for p in params] + [sympy.diff(v, p) for p in params] + [sympy.diff(P[2], p) for p in params]
    return sympy.lambdify(params + (px, py, pz, fx, fy, ox, oy), out, "math")
