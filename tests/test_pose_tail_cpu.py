"""The trajectory tail -- phovo_trajectory_chain, phovo_trajectory_format_pose (csrc/trajectory.cpp over
include/phovo/compat/Numeric.h's inverse() and Quaternion) and the three system-line formatters -- against the mpmath
checker of tests/pose_tail.py, through native.lib().  No device.

Every directed case asserts that it reached its edge: the row swaps taken (pose_tail.pivots), the quaternion branch
(pose_tail.quaternion_branch), the byte at which a buffer is exactly full.  Every test prints what it measured against its
bar; the bars are pose_tail's.
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

import pose_tail as pt

import phovo_amd  # noqa: F401
from phovo_amd import native, se3, sequence

DP = pt.DP


# ------------------------------------------------------------------------------------------------------------------------
# inverse()
# ------------------------------------------------------------------------------------------------------------------------
def _inverse_errors(states):
    """One chain step from the identity is Rt^-1 itself (the product with I is exact).  Returns (worst error, pivots)."""
    worst, taken = 0.0, []
    for s in states:
        rt = pt.eigen_pose(s)
        single, _ = pt.chain([s])
        err = pt.worst_error(single[0], pt.exact_inverse(rt))
        assert err <= pt.INVERSE_BAR, (list(s), err)
        worst = max(worst, err)
        taken.append(pt.pivots(rt))
    return worst, taken


def test_inverse_at_the_row_swaps():
    states = pt.directed_states()
    worst, taken = _inverse_errors(states)
    by_state = {tuple(s[3:]): p for s, p in zip(states, taken)}
    e, q = 1e-9, pt.PI / 4
    # |R10| > |R00| just beyond a yaw of 45 degrees and not just before; up to 135 degrees; not at 180
    assert by_state[(q + e, 0.0, 0.0)][0] == 1 and by_state[(q - e, 0.0, 0.0)][0] == 0
    assert by_state[(-(q + e), 0.0, 0.0)][0] == 1 and by_state[(-(q - e), 0.0, 0.0)][0] == 0
    assert by_state[(pt.PI / 2, 0.0, 0.0)][0] == 1 and by_state[(pt.PI, 0.0, 0.0)][0] == 0
    # a pitch of +-90 degrees leaves R00 = cos(pi/2) = 6e-17 and R20 = -+1: the third row is the pivot
    assert by_state[(0.0, pt.PI / 2, 0.0)][0] == 2 and by_state[(0.0, -pt.PI / 2, 0.0)][0] == 2
    assert abs(pt.eigen_pose([0, 0, 0, 0, pt.PI / 2, 0])[0, 0]) < 1e-16
    # a roll of +-90 degrees: R11 = 6e-17, R21 = +-1: a swap at the second step
    assert by_state[(0.0, 0.0, pt.PI / 2)][:2] == (0, 2) and by_state[(0.0, 0.0, -pt.PI / 2)][:2] == (0, 2)
    print(f"inverse, {len(states)} directed states: worst {worst:.3e}, bar {pt.INVERSE_BAR:.1e} ({worst / pt.INVERSE_BAR:.3f})")


def test_inverse_seeded():
    states = pt.seeded_states()
    assert len(states) == 3000 and np.abs(states[:, :3]).max() <= 1 and np.abs(states[:, 3:]).max() <= pt.PI
    worst, taken = _inverse_errors(states)
    # both outcomes at every step at which a swap is possible: step 0 (rows 1 or 2) and step 1 (row 2).  At steps 2 and 3
    # the rows below hold (0 0 0 1): no swap exists.
    step0 = [p[0] for p in taken]
    step1 = [p[1] for p in taken]
    assert all(p[2:] == (2, 3) for p in taken)
    counts = {"step 0 keeps": step0.count(0), "step 0 takes row 1": step0.count(1), "step 0 takes row 2": step0.count(2),
              "step 1 keeps": step1.count(1), "step 1 takes row 2": step1.count(2)}
    assert min(counts.values()) >= 300, counts
    print(f"inverse, 3000 seeded states: worst {worst:.3e}, bar {pt.INVERSE_BAR:.1e} ({worst / pt.INVERSE_BAR:.3f}); {counts}")


# ------------------------------------------------------------------------------------------------------------------------
# Quaternion(R)
# ------------------------------------------------------------------------------------------------------------------------
def _hold_quaternion(R, exact, branch, what):
    """The printed quaternion and se3.rotation_to_quaternion against the exact one: in the convention, equal within the bar
    (which makes the common sign the convention's), of unit length within the bar.  Returns the worst error."""
    want = pt.in_convention(exact, branch)
    worst = 0.0
    for name, got in (("C++", pt.printed_quaternion(R)), ("se3", tuple(se3.rotation_to_quaternion(np.asarray(R))))):
        lead = got[3] if branch == 0 else got[branch - 1]
        assert lead >= 0 if branch == 0 else lead > 0, (what, name, branch, got)
        with mpmath.workdps(pt.DPS):
            for g, w in zip(got, want):
                err = float(abs(mpmath.mpf(float(g)) - w))
                assert err <= pt.quaternion_bar(w), (what, name, branch, got, [float(v) for v in want], err)
                worst = max(worst, err)
            norm = float(abs(mpmath.sqrt(sum(mpmath.mpf(float(g)) ** 2 for g in got)) - 1))
        assert norm <= pt.quaternion_bar(1.0), (what, name, norm)
    return worst


def test_quaternion_exact_rotations():
    half = mpmath.mpf(1) / 2
    cases = [(np.eye(3), (0, 0, 0, 1), 0), (np.diag([1.0, -1, -1]), (1, 0, 0, 0), 1), (np.diag([-1.0, 1, -1]), (0, 1, 0, 0), 2),
             (np.diag([-1.0, -1, 1]), (0, 0, 1, 0), 3),
             (np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]), (half, half, half, half), 1),        # trace exactly 0: not > 0
             (np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), (half, half, half, -half), 1)]       # its transpose
    for R, exact, branch in cases:
        assert pt.quaternion_branch(R) == branch, R
        exact = tuple(mpmath.mpf(v) for v in exact)
        assert pt.in_convention(exact, branch) == exact                  # the stated answers are in the convention as they stand
        assert _hold_quaternion(R, exact, branch, R.tolist()) == 0.0     # exact inputs, exact answers
        assert pt.printed_quaternion(R) == tuple(float(v) for v in exact)
    cube = pt.cube_rotations()
    assert len(cube) == 24
    seen = set()
    for R, exact, turns in cube:
        assert np.array_equal(R @ R.T, np.eye(3)) and round(np.linalg.det(R)) == 1
        b = pt.quaternion_branch(R)
        seen.add(b)
        _hold_quaternion(R, exact, b, turns)
    assert seen == {0, 1, 2, 3}


def test_quaternion_seeded():
    states = pt.seeded_states()
    counts, worst = [0, 0, 0, 0], 0.0
    for s in states:
        R = pt.eigen_pose(s)[:3, :3]
        b = pt.quaternion_branch(R)
        counts[b] += 1
        worst = max(worst, _hold_quaternion(R, pt.euler_quaternion(*s[3:]), b, list(s)))
    assert min(counts) >= 400, counts
    print(f"quaternion, 3000 seeded rotations: worst {worst:.3e}, bar {pt.quaternion_bar(1.0):.3e} at |q| = 1; "
          f"branches {counts}")


# ------------------------------------------------------------------------------------------------------------------------
# the chain
# ------------------------------------------------------------------------------------------------------------------------
def test_chain_of_216_steps_through_every_branch():
    states = pt.chain_states()
    assert states.shape == (216, 6)
    poses, last = pt.chain(states)
    exact = pt.exact_chain([pt.eigen_pose(s) for s in states])
    worst, branches = 0.0, set()
    ts = 1305031102.175304 + 0.033 * np.arange(1, 217)
    lines = []
    for p, e, t in zip(poses, exact, ts):
        err = pt.worst_error(p, e)
        assert err <= pt.CHAIN_BAR, err
        worst = max(worst, err)
        branches.add(pt.quaternion_branch(p[:3, :3]))
        line = pt.format_pose(t, p)
        lines.append(line)
        f = [float(v) for v in line.split()]
        assert len(f) == 8 and abs(f[0] - t) <= 5e-16 * abs(t)
        for got, want in zip(f[1:4], p[:3, 3]):
            assert abs(got - want) <= 5e-16 * abs(want), (got, want)
    assert branches == {0, 1, 2, 3}, branches
    tmax = float(np.abs(poses[:, :3, 3]).max())
    print(f"chain, 216 steps, |t| up to {tmax:.2f}: worst {worst:.3e}, bar {pt.CHAIN_BAR:.0e} ({worst / pt.CHAIN_BAR:.4f})")
    assert np.array_equal(last, poses[-1])
    # three calls == one call, bit for bit
    a, pa = pt.chain(states[:72])
    b, pb = pt.chain(states[72:150], pa)
    c, pc = pt.chain(states[150:], pb)
    assert np.array_equal(np.concatenate([a, b, c]), poses) and np.array_equal(pc, last)
    # the file the sequence driver writes is these lines
    text = sequence.chain_and_format(states, ts)
    assert text == "\n".join(["# estimated trajectory", "# timestamp tx ty tz qx qy qz qw"] + lines) + "\n"
    assert text.encode() == text.encode("ascii")


def test_chain_of_nothing_and_its_refusals():
    L = native.lib()
    pose = np.arange(16, dtype=np.float64)
    keep = pose.copy()
    assert L.phovo_trajectory_chain(0, None, pose.ctypes.data_as(DP), None) == 0
    assert np.array_equal(pose, keep)
    assert L.phovo_trajectory_chain(-1, None, pose.ctypes.data_as(DP), None) != 0
    st = np.zeros(6)
    assert L.phovo_trajectory_chain(-1, st.ctypes.data, pose.ctypes.data_as(DP), None) != 0
    assert L.phovo_trajectory_chain(1, None, pose.ctypes.data_as(DP), None) != 0
    assert L.phovo_trajectory_chain(1, st.ctypes.data, None, None) != 0
    assert np.array_equal(pose, keep)


# ------------------------------------------------------------------------------------------------------------------------
# the four line formatters at their exact capacity
# ------------------------------------------------------------------------------------------------------------------------
GUARD = 0xAA


def _fresh(n):
    buf = (C.c_char * n)()
    C.memset(buf, GUARD, n)
    return buf


def _values(rs, n):
    """Doubles whose %.17g form is long: signs, 17 digits and three-digit exponents among them."""
    v = rs.uniform(-1, 1, n) * 10.0 ** rs.randint(-300, 300, n)
    v[::5] = rs.uniform(-1e3, 1e3, len(v[::5]))
    return v


def _fill(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = float(v)


def _formatters():
    rs = np.random.RandomState(8)
    pose = pt.chain(pt.chain_states()[:100])[1].reshape(16)
    pair = native.PairSystem()
    _fill(pair.information, _values(rs, 36))
    pair.cost, pair.rows = float(_values(rs, 1)[0]), 307200
    sampled = []
    for dim in (6, 8):
        s = native.SampledSystem()
        _fill(s.information, _values(rs, 64))
        s.cost, s.rows, s.dim = float(_values(rs, 1)[0]), 76800, dim
        sampled.append(s)
    geo = native.GeometricSystem()
    _fill(geo.photometric_information, _values(rs, 36))
    _fill(geo.depth_information, _values(rs, 36))
    geo.photometric_cost, geo.depth_cost, geo.rows, geo.depth_rows = 1.0 / 3, -2e-300 / 3, 2147483647, -2147483647
    L = native.lib()
    ts = 1305031102.175304
    return [("pose", lambda b, n: L.phovo_trajectory_format_pose(ts, pose.ctypes.data_as(DP), b, n), 8, 1),
            ("pair", lambda b, n: L.phovo_pair_system_format(ts, C.byref(pair), b, n), 24, 1),
            ("sampled 6", lambda b, n: L.phovo_sampled_system_format(ts, C.byref(sampled[0]), b, n), 25, 1),
            ("sampled 8", lambda b, n: L.phovo_sampled_system_format(ts, C.byref(sampled[1]), b, n), 40, 1),
            ("geometric", lambda b, n: L.phovo_geometric_system_format(ts, C.byref(geo), b, n), 47,
             native.GEOMETRIC_SYSTEM_LINE_CAPACITY)]


@pytest.mark.parametrize("index", range(5), ids=["pose", "pair", "sampled6", "sampled8", "geometric"])
def test_formatters_at_their_exact_capacity(index):
    """capacity = length + 1 succeeds and writes exactly length + 1 bytes; capacity = length is refused with the buffer
    untouched.  phovo_geometric_system_format asks for PHOVO_GEOMETRIC_SYSTEM_LINE_CAPACITY whatever the line needs (its
    lines are always shorter), so its edge is that constant against one less."""
    name, call, fields, floor = _formatters()[index]
    big = _fresh(4096)
    assert call(big, 4096) == 0
    line = big.value
    n = len(line)
    assert len(line.split()) == fields and bytes(big)[n] == 0 and set(bytes(big)[n + 1:]) == {GUARD}
    enough = max(n + 1, floor)
    assert floor == 1 or n + 1 < floor                               # the geometric line never needs its whole capacity
    buf = _fresh(enough + 32)
    assert call(buf, enough) == 0, name
    raw = bytes(buf)
    assert raw[:n] == line and raw[n] == 0 and set(raw[n + 1:]) == {GUARD}, name      # length + 1 bytes, nothing behind
    buf = _fresh(enough + 32)
    assert call(buf, enough - 1) != 0, name
    assert native.lib().phovo_last_error(), name
    assert set(bytes(buf)) == {GUARD}, name                          # refused: untouched
    assert call(buf, 0) != 0 and set(bytes(buf)) == {GUARD}, name
    # %.17g round-trips: the line reparses to the numbers it was made from (the pose line prints 16 digits)
    if name != "pose":
        assert float(line.split()[0]) == 1305031102.175304


def test_sampled_system_format_refuses_a_dim_of_7():
    s = native.SampledSystem()
    buf = _fresh(4096)
    for dim, ok in ((6, True), (8, True), (7, False), (0, False), (-6, False), (9, False)):
        s.dim = dim
        C.memset(buf, GUARD, 4096)
        assert (native.lib().phovo_sampled_system_format(1.0, C.byref(s), buf, 4096) == 0) == ok, dim
        assert ok or set(bytes(buf)) == {GUARD}


def test_formatters_refuse_null():
    L = native.lib()
    buf = _fresh(2048)
    pose = np.eye(4).reshape(16)
    assert L.phovo_trajectory_format_pose(1.0, None, buf, 2048) != 0
    assert L.phovo_trajectory_format_pose(1.0, pose.ctypes.data_as(DP), None, 2048) != 0
    assert L.phovo_pair_system_format(1.0, None, buf, 2048) != 0
    assert L.phovo_sampled_system_format(1.0, None, buf, 2048) != 0
    assert L.phovo_geometric_system_format(1.0, None, buf, 2048) != 0
    assert set(bytes(buf)) == {GUARD}


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_pose_that_is_not_finite_formats_and_reparses_as_such(bad):
    pose = np.full((4, 4), bad)
    line = pt.format_pose(bad, pose)
    f = [float(v) for v in line.split()]
    assert len(f) == 8 and not np.isfinite(f).any()
    pose = np.eye(4)
    pose[0, 3], pose[1, 1] = bad, bad                                # one translation, one rotation entry
    f = [float(v) for v in pt.format_pose(1.0, pose).split()]
    assert len(f) == 8 and f[0] == 1.0 and not np.isfinite(f[1]) and np.isfinite(f[2:4]).all()
    assert not np.isfinite(f[4:]).all()
