"""An independent checker for the trajectory tail (csrc/trajectory.cpp, include/phovo/compat/Numeric.h: inverse(),
Quaternion) and the states that drive it.  No device.

The checker works in mpmath at 60 digits and restates nothing of Numeric.h:
  * the inverse of a binary64 4x4 matrix is mpmath's, taken as exact; a chain is the product of such inverses;
  * the quaternion of R = Rz(yaw) Ry(pitch) Rx(roll) comes from the angles, as the product of the three half-angle
    quaternions, not from the matrix.
Two rules of the code under test are restated once each, only to say which path an input takes (coverage, never an
expectation): the partial-pivoting rule of inverse() (`pivots`, in exact rational arithmetic) and the branch choice of
Quaternion(R) (`quaternion_branch`).
"""
import ctypes as C
from fractions import Fraction

import mpmath
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import native

DPS = 60
DP = C.POINTER(C.c_double)

# The bars.  A numpy emulation of the Gauss-Jordan stayed within 4.3e-16 of the exact inverse on these
# states; the compiled code is held to 16 times that.  The quaternion: 8 ulp of 1 plus the 16 significant digits of the line.
INVERSE_BAR = 7e-15
CHAIN_BAR = 1e-12                    # the project's own (tests/test_sequence_sharded.py)


def quaternion_bar(q):
    return 8 * 2.0 ** -52 + 5e-16 * abs(float(q))


# ------------------------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------------------------
def mp_matrix(m):
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in np.asarray(m).reshape(4, 4)])


def exact_inverse(m):
    with mpmath.workdps(DPS):
        return mpmath.inverse(mp_matrix(m))


def exact_chain(rts, pose=None):
    """pose_t = pose_{t-1} Rt_t^-1 for binary64 Rt, at 60 digits.  Returns the list of poses."""
    with mpmath.workdps(DPS):
        p = mpmath.eye(4) if pose is None else mp_matrix(pose)
        out = []
        for rt in rts:
            p = p * mpmath.inverse(mp_matrix(rt))
            out.append(p.copy())
        return out


def worst_error(got, exact):
    """max |got - exact| over the 16 entries, as a float."""
    with mpmath.workdps(DPS):
        g = np.asarray(got).reshape(4, 4)
        return float(max(abs(mpmath.mpf(float(g[i, j])) - exact[i, j]) for i in range(4) for j in range(4)))


def _half_angle_quaternion(hy, hp, hr):
    cy, sy, cp, sp, cr, sr = mpmath.cos(hy), mpmath.sin(hy), mpmath.cos(hp), mpmath.sin(hp), mpmath.cos(hr), mpmath.sin(hr)
    return (cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr,
            cy * cp * cr + sy * sp * sr)


def euler_quaternion(yaw, pitch, roll):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll) = qz * qy * qx, from the half angles of the binary64 angles."""
    with mpmath.workdps(DPS):
        return _half_angle_quaternion(*(mpmath.mpf(float(a)) / 2 for a in (yaw, pitch, roll)))


def quaternion_branch(R):
    """0: trace > 0; 1, 2, 3: the largest diagonal entry is R00, R11, R22 (the later one only where strictly larger)."""
    R = np.asarray(R)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return 1 + i


def in_convention(q, branch):
    """q or -q: w >= 0 in the trace branch, the component of the largest diagonal entry > 0 in the others."""
    lead = q[3] if branch == 0 else q[branch - 1]
    return tuple(-v for v in q) if lead < 0 else tuple(q)


def pivots(m):
    """The pivot row partial pivoting takes at each elimination step of a Gauss-Jordan on m, in exact arithmetic: the first
    row at or below the diagonal whose entry in column k is strictly largest in size."""
    a = [[Fraction(float(v)) for v in row] for row in np.asarray(m).reshape(4, 4)]
    out = []
    for k in range(4):
        piv = k
        for r in range(k + 1, 4):
            if abs(a[r][k]) > abs(a[piv][k]):
                piv = r
        out.append(piv)
        a[k], a[piv] = a[piv], a[k]
        a[k] = [v / a[k][k] for v in a[k]]
        for r in range(4):
            if r != k:
                f = a[r][k]
                a[r] = [x - f * y for x, y in zip(a[r], a[k])]
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------
# the code under test, through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def eigen_pose(state):
    s = np.ascontiguousarray(state, dtype=np.float64)
    rt = np.zeros(16)
    native.check(native.lib().phovo_eigen_pose(s.ctypes.data_as(DP), rt.ctypes.data_as(DP)), "phovo_eigen_pose")
    return rt.reshape(4, 4)


def chain(states, pose=None):
    """phovo_trajectory_chain: ([n, 4, 4] poses, final pose)."""
    states = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 6)
    n = states.shape[0]
    io = (np.eye(4) if pose is None else np.array(pose, dtype=np.float64)).reshape(16).copy()
    poses = np.zeros((max(n, 1), 16))
    native.check(native.lib().phovo_trajectory_chain(n, states.ctypes.data, io.ctypes.data_as(DP), poses.ctypes.data),
                 "phovo_trajectory_chain")
    return poses[:n].reshape(n, 4, 4), io.reshape(4, 4)


def format_pose(timestamp, pose):
    buf = C.create_string_buffer(256)
    p = np.ascontiguousarray(pose, dtype=np.float64).reshape(16)
    native.check(native.lib().phovo_trajectory_format_pose(float(timestamp), p.ctypes.data_as(DP), buf, len(buf)),
                 "phovo_trajectory_format_pose")
    return buf.value.decode()


def printed_quaternion(R):
    """(x, y, z, w) as phovo_trajectory_format_pose prints it for the rotation R."""
    pose = np.eye(4)
    pose[:3, :3] = R
    return tuple(float(v) for v in format_pose(0.0, pose).split()[4:8])


# ------------------------------------------------------------------------------------------------------------------------
# states
# ------------------------------------------------------------------------------------------------------------------------
PI = float(np.pi)


def _angle_edges(quarter):
    """The angles at which a row swap (or a quaternion branch) changes hands for one axis."""
    e = 1e-9
    if quarter:                                                    # yaw: |R10| = |R00| at pi/4 and 3 pi/4
        return [s * (PI / 4 + d) for s in (1, -1) for d in (e, -e)] + [PI / 2, -PI / 2, 3 * PI / 4, -3 * PI / 4, PI]
    return [PI / 2, -PI / 2, PI / 2 - e, -(PI / 2 - e)]           # pitch, roll: R00 (R11) about 6e-17


def directed_states():
    yaw, pitch, roll = _angle_edges(True), _angle_edges(False), _angle_edges(False)
    t = [0.25, -0.5, 1.0]
    out = [t + [a, 0.0, 0.0] for a in yaw] + [t + [0.0, a, 0.0] for a in pitch] + [t + [0.0, 0.0, a] for a in roll]
    out += [t + [a, b, 0.0] for a in yaw for b in pitch] + [t + [a, 0.0, c] for a in yaw for c in roll]
    out += [t + [0.0, b, c] for b in pitch for c in roll]
    return np.array(out)


def seeded_states(n=3000, seed=4711):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.uniform(-1, 1, (n, 3)), rs.uniform(-PI, PI, (n, 3))], axis=1)


def chain_states(seed=216):
    """216 steps: 72 of 5 degrees of yaw, 72 of pitch, 72 of roll, the other angles and the translation small (<= 0.05)."""
    rs = np.random.RandomState(seed)
    st = rs.uniform(-0.05, 0.05, (216, 6))
    for leg, axis in enumerate((3, 4, 5)):
        st[72 * leg:72 * (leg + 1), axis] = np.deg2rad(5.0)
    return st


def cube_rotations():
    """The 24 rotations of the cube as (integer matrix, exact quaternion from the angles, angles in quarter turns): every
    R = Rz(a) Ry(b) Rx(c) with quarter-turn angles, each matrix once."""
    cs, sn = [1, 0, -1, 0], [0, 1, 0, -1]
    seen = {}
    for a in range(4):
        for b in range(4):
            for c in range(4):
                cy, sy, cp, sp, cr, sr = cs[a], sn[a], cs[b], sn[b], cs[c], sn[c]
                R = ((cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr),
                     (sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr),
                     (-sp, cp * sr, cp * cr))
                if R not in seen:
                    with mpmath.workdps(DPS):
                        q = _half_angle_quaternion(a * mpmath.pi / 4, b * mpmath.pi / 4, c * mpmath.pi / 4)
                    seen[R] = (np.array(R, dtype=np.float64), q, (a, b, c))
    return list(seen.values())
