"""write_pose_constants (csrc/gn_device.hpp) on the device, against exact arithmetic.

Every Gauss-Newton kernel form starts an iteration with it: (yaw, pitch, roll) -> sin / cos -> the 23 pose constants.  The
device has three ways to the sines and cosines, chosen per wave (lanes 0, 1, 2 take yaw, pitch, roll; lanes 3.. yaw):
  branch 1  |a| < 0.3 on every lane:             fdlibm's __kernel_sin / __kernel_cos polynomials, cos summed naively,
  branch 2  0.3 <= |a| <= fl(pi/4) on every lane: the same polynomials, cos with fdlibm's qx taken out of both big terms,
  branch 3  any lane beyond fl(pi/4), or NaN:     the device library's sincos, for all three angles.
tests/native/pose_constants_probe.hip runs the header's function unchanged, one wave per state; this file holds what it
returns to
  * exact sin / cos of the double angles (mpmath, 128 bits): at most 1 ulp in branches 1 and 2, at most 2 ulp in branch 3
    (an assumed bar for the library's sincos; the measured maxima are printed),
  * a bit-exact CPU emulation of branches 1 and 2 (exact fma): the compiled code is the algorithm the source states,
  * the reference's formulas for the composite constants (...Analytic.h:219-266, temp11's `+ x` included) evaluated
    exactly, with a bar derived from the factors' bars and the rounding operations of each formula,
  * NaN / inf in one angle: exactly the constants that depend on it are NaN.
"""
import ctypes
import functools
import math
import os
import struct
import subprocess
from fractions import Fraction

import mpmath
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")

NAMES = ["X", "Y", "Z", "R01", "R02", "R11", "R12", "T1", "T2", "T3", "T4", "T5", "T6", "T8", "T11", "T14", "T15",
         "T16", "T17", "T24", "CY", "SY"]                       # the enum of gn_device.hpp, in order
IDX = {n: i for i, n in enumerate(NAMES)}
P4 = 0.78539816339744828                                        # fl(pi/4): the ballot's bound
U = 2.0 ** -53
ULP_BAR = {1: 1.0, 2: 1.0, 3: 2.0}

# Each composite constant as the reference writes it: monomials of (sy, cy, sp, cp, sr, cr) with their signs, whether x is
# added (temp11), and the number of rounding operations (multiplies and adds) the formula has.
COMPOSITES = {
    "R01": ([(+1, "cy sp sr"), (-1, "sy cr")], False, 4),
    "R02": ([(+1, "cy sp cr"), (+1, "sy sr")], False, 4),
    "R11": ([(+1, "sy sp sr"), (+1, "cy cr")], False, 4),
    "R12": ([(+1, "sy sp cr"), (-1, "cy sr")], False, 4),
    "T1": ([(+1, "cp sr")], False, 1),
    "T2": ([(+1, "cp cr")], False, 1),
    "T4": ([(+1, "sr sy"), (+1, "sp cr cy")], False, 4),
    "T5": ([(+1, "sp sr cy"), (-1, "cr sy")], False, 4),
    "T6": ([(+1, "sp sr sy"), (+1, "cr cy")], False, 4),
    "T8": ([(+1, "sr cy"), (-1, "sp cr sy")], False, 4),
    "T11": ([(+1, "cp cy")], True, 2),
    "T14": ([(+1, "cp sy")], False, 1),
    "T15": ([(+1, "cp cy")], False, 1),
    "T16": ([(+1, "sp sr")], False, 1),
    "T17": ([(+1, "sp cr")], False, 1),
}
# which angles each constant depends on (yaw, pitch, roll)
DEPENDS = {"X": "", "Y": "", "Z": "", "T3": "p", "T24": "p", "CY": "y", "SY": "y"}
for _n, (_m, _x, _ops) in COMPOSITES.items():
    DEPENDS[_n] = "".join(sorted({f[1] for _s, mono in _m for f in mono.split()}, key="ypr".index))


# ------------------------------------------------------------------------------------------------------------------------
# exact reference values and the CPU emulation of branches 1 and 2
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_sincos(a):
    with mpmath.workprec(128):
        x = mpmath.mpf(a)
        return mpmath.sin(x), mpmath.cos(x)


def ulp_of(v):
    """Spacing of the doubles at the exact value v (2^-1074 at and below the subnormal range)."""
    if v == 0:
        return mpmath.mpf(2) ** -1074
    _, e = mpmath.frexp(v)                       # |v| in [2^(e-1), 2^e)
    return mpmath.mpf(2) ** max(int(e) - 53, -1074)


def ulp_error(dev, exact):
    with mpmath.workprec(128):
        return float(abs(mpmath.mpf(dev) - exact) / ulp_of(exact))


def _fma(a, b, c):
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r != 0 else (a * b + c)  # exact zero: the IEEE sign rule, which a * b + c applies exactly


def _hi_minus(ax, d):
    hi = struct.unpack("<Q", struct.pack("<d", ax))[0] >> 32
    return struct.unpack("<d", struct.pack("<Q", (hi - d) << 32))[0]


SIN_COEF = [1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06,
            -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01]
COS_COEF = [-1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07,
            2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02]


def emulate_polynomial(a):
    """Branches 1 and 2 of write_pose_constants, operation for operation, every fma exact-then-rounded."""
    z = a * a
    ps = _fma(z, SIN_COEF[0], SIN_COEF[1])
    pc = _fma(z, COS_COEF[0], COS_COEF[1])
    for s, c in zip(SIN_COEF[2:], COS_COEF[2:]):
        ps, pc = _fma(z, ps, s), _fma(z, pc, c)
    sn = _fma(a * z, ps, a)
    ax = abs(a)
    qx = 0.0 if ax < 0.3 else (0.28125 if ax > 0.78125 else _hi_minus(ax, 0x00200000))
    cs = (1.0 - qx) - _fma(-z, z * pc, 0.5 * z - qx)
    return sn, cs


def branch_of_state(yaw, pitch, roll):
    if not all(abs(a) <= P4 for a in (yaw, pitch, roll)):       # NaN compares false: branch 3 as on the device
        return 3
    return None                                                 # 1 or 2, per angle


def branch_of_angle(a, state_branch):
    return state_branch or (1 if abs(a) < 0.3 else 2)


def composite_exact_and_bar(name, sc, x, b):
    """Exact value of a composite constant and its bar: a formula of monomials whose K <= 3 sin / cos factors each carry a
    relative error of at most b ulp <= 2 b u (u = 2^-53), evaluated with n rounding operations of relative error u each:
        |device - exact| <= ((1 + 2 b u)^K (1 + u)^n - 1) * sum |monomials| + n * 2^-1075
    (the last term: absolute rounding of results in the subnormal range)."""
    monos, plus_x, n = COMPOSITES[name]
    with mpmath.workprec(128):
        val, mag, k = mpmath.mpf(0), mpmath.mpf(0), 0
        for sign, mono in monos:
            t = mpmath.mpf(sign)
            for f in mono.split():
                t *= sc[f]
            k = max(k, len(mono.split()))
            val += t
            mag += abs(t)
        if plus_x:
            val += mpmath.mpf(x)
            mag += abs(mpmath.mpf(x))
        u = mpmath.mpf(2) ** -53
        bar = ((1 + 2 * b * u) ** k * (1 + u) ** n - 1) * mag + n * mpmath.mpf(2) ** -1075
        return val, bar


# ------------------------------------------------------------------------------------------------------------------------
# the angles
# ------------------------------------------------------------------------------------------------------------------------
def _next(a, k=1):
    for _ in range(abs(k)):
        a = float(np.nextafter(a, math.inf if k > 0 else -math.inf))
    return a


FDLIBM_03 = struct.unpack("<d", struct.pack("<Q", 0x3FD33333 << 32))[0]     # first double with fdlibm's high word of 0.3
SMALL_SPECIAL = ([0.0, 5e-324, 1e-300, 2.0 ** -27, 0.3, FDLIBM_03, 0.78125, P4]
                 + [_next(0.3, k) for k in (-3, -2, -1, 1, 2, 3)] + [_next(FDLIBM_03, k) for k in (-1, 1)]
                 + [_next(0.78125, -1), _next(0.78125, 1), _next(P4, -1)])
LARGE = [_next(P4, 1), 0.79, 1.0, 1.5707963267948966, 2.0, 3.141592653589793, 6.3, 100.0, 1e5, 2.0 ** 30]


def small_magnitudes():
    dense = np.linspace(0.0, P4, 1025)
    top = np.linspace(0.78125, P4, 514)[1:]                     # 513 points in (0.78125, fl(pi/4)]
    return sorted(set(float(v) for v in np.concatenate([dense, top])) | set(SMALL_SPECIAL))


XYZ = (0.125, -0.375, 1.75)


def states_for(mags):
    """Four states per magnitude a: yaw and roll of both signs with pitch = 0 (then C_T1 = sr, C_T2 = cr exactly), and
    all three angles at +a and at -a (pitch of both signs, every composite with three non-trivial factors)."""
    out = []
    for a in mags:
        out += [(a, 0.0, -a), (-a, 0.0, a), (a, a, a), (-a, -a, -a)]
    return out


def mixed_states():
    """One angle beyond pi/4 and the others small: the small ones take branch 3 (each lane role raises the ballot once)."""
    smalls = [0.0, 1e-300, 2.0 ** -27, 0.01, 0.29, 0.3, FDLIBM_03, 0.55, 0.78125, P4]
    out = []
    for big in LARGE:
        for s in smalls:
            for sg in (1.0, -1.0):
                out += [(sg * big, sg * s, 0.0), (sg * big, 0.0, -sg * s),      # big yaw (lanes 0, 3..63)
                        (sg * s, sg * big, 0.0),                                 # big pitch (lane 1)
                        (-sg * s, 0.0, sg * big)]                                # big roll (lane 2)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the probe
# ------------------------------------------------------------------------------------------------------------------------
def build_probe(build_dir=None):
    args = ["make", "-s", "-C", CSRC, "pose-probe"] + ([f"BUILD={build_dir}"] if build_dir else [])
    subprocess.check_call(args)
    return os.path.join(build_dir or os.path.join(CSRC, "build"), "pose_constants_probe.so")


@pytest.fixture(scope="module")
def probe():
    lib = ctypes.CDLL(build_probe())
    lib.pose_probe_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert lib.pose_probe_count() == len(NAMES)

    def run(states):
        st = np.ascontiguousarray(np.array([XYZ + tuple(s) for s in states], dtype=np.float64))
        out = np.zeros((len(states), len(NAMES)))
        assert lib.pose_probe_run(st.ctypes.data, len(states), out.ctypes.data) == 0
        return out
    return run


def sincos_from_row(row, state):
    """Device sin / cos per angle as read straight from the constants: yaw from C_SY / C_CY, pitch from C_T3 / C_T24,
    roll from C_T1 / C_T2 where pitch = 0."""
    yaw, pitch, roll = state
    got = [("yaw", yaw, row[IDX["SY"]], row[IDX["CY"]]), ("pitch", pitch, row[IDX["T3"]], row[IDX["T24"]])]
    if pitch == 0.0:
        got.append(("roll", roll, row[IDX["T1"]], row[IDX["T2"]]))
    return got


def check_rows(states, rows):
    """Every sin / cos against its branch's ulp bar and the emulation, every composite against its bar.  Returns the
    worst ulp error per branch and the worst composite error / bar."""
    worst = {1: [0.0, 0.0], 2: [0.0, 0.0], 3: [0.0, 0.0]}
    worst_ratio, fails = 0.0, []
    for state, row in zip(states, rows):
        sb = branch_of_state(*state)
        assert tuple(row[:3]) == XYZ
        for axis, a, s, c in sincos_from_row(row, state):
            br = branch_of_angle(a, sb)
            es, ec = exact_sincos(a)
            us, uc = ulp_error(s, es), ulp_error(c, ec)
            worst[br][0], worst[br][1] = max(worst[br][0], us), max(worst[br][1], uc)
            if us > ULP_BAR[br] or uc > ULP_BAR[br]:
                fails.append(f"{axis} {a!r} branch {br}: sin {us:.3f} ulp, cos {uc:.3f} ulp")
            if br < 3 and (s, c) != emulate_polynomial(a):
                fails.append(f"{axis} {a!r} branch {br}: device ({s!r}, {c!r}) != emulation {emulate_polynomial(a)!r}")
        b = max(ULP_BAR[branch_of_angle(a, sb)] for a in state)
        sc = {}
        for k, a in zip("ypr", state):
            sc["s" + k], sc["c" + k] = exact_sincos(a)
        for name in COMPOSITES:
            val, bar = composite_exact_and_bar(name, sc, XYZ[0], b)
            err = abs(mpmath.mpf(row[IDX[name]]) - val)
            worst_ratio = max(worst_ratio, float(err / bar))
            if err > bar:
                fails.append(f"{name} at {state!r}: error {float(err):.3e} > bar {float(bar):.3e}")
    assert not fails, f"{len(fails)} misses, first ones:\n" + "\n".join(fails[:20])
    return worst, worst_ratio


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the probe builds; the polynomial branches are what the source's comments claim
# ------------------------------------------------------------------------------------------------------------------------
def test_pose_probe_builds_out_of_the_product_library(tmp_path):
    """`make pose-probe` compiles the probe against the header as it stands, into the build directory given, and nothing
    of it reaches the product library."""
    so = build_probe(str(tmp_path))
    assert os.path.exists(so)
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "pose_probe_run") and hasattr(lib, "pose_probe_count")
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "photoconsistency-visual-odometry_amd",
                                                                    "libphovo_hip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        assert "pose_probe" not in nm.stdout
    assert not any(f.startswith("pose_constants_probe") for f in os.listdir(os.path.dirname(CSRC)))


def test_polynomial_branches_emulated_on_the_cpu_are_within_one_ulp():
    """The algorithm of branches 1 and 2 (emulated with exact fma) against 128-bit sin / cos over the dense sweep of
    [0, fl(pi/4)] and the threshold neighbourhoods, both signs: under one ulp, i.e. what the device must reproduce."""
    worst = [0.0, 0.0]
    for m in small_magnitudes():
        for a in (m, -m):
            s, c = emulate_polynomial(a)
            es, ec = exact_sincos(a)
            worst = [max(worst[0], ulp_error(s, es)), max(worst[1], ulp_error(c, ec))]
    print(f"emulated polynomial: sin {worst[0]:.3f} ulp, cos {worst[1]:.3f} ulp at worst")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pose_constants_on_every_branch(probe):
    """The dense sweep of [-fl(pi/4), fl(pi/4)] (513 points inside (0.78125, fl(pi/4)]), the thresholds 0.3 (and fdlibm's
    own, high word 0x3FD33333), 0.78125, fl(pi/4) and their neighbours, zero, subnormal and tiny angles -- branches 1 and 2
    -- and 0.79 ... 2^30 -- branch 3 -- on each axis, both signs."""
    states = states_for(small_magnitudes() + LARGE)
    worst, ratio = check_rows(states, probe(states))
    for br in (1, 2, 3):
        print(f"branch {br}: sin {worst[br][0]:.3f} ulp, cos {worst[br][1]:.3f} ulp at worst (bar {ULP_BAR[br]:g})")
    print(f"composite constants: worst error / bar {ratio:.3f}")
    assert all(worst[br][0] > 0 or worst[br][1] > 0 for br in (1, 2, 3))     # every branch was measured


@pytest.mark.gpu
def test_pose_constants_in_mixed_waves(probe):
    """One angle beyond pi/4 raises the ballot from its lane: the small angles of the same state take the library's
    sincos and meet branch 3's bar; all three angles at fl(pi/4) stay on the polynomials (branch 2, bit for bit the
    emulation)."""
    states = mixed_states() + [(P4, P4, P4), (-P4, -P4, -P4), (P4, 0.0, -P4), (-P4, 0.0, P4)]
    worst, ratio = check_rows(states, probe(states))
    print(f"small angles in branch 3: sin {worst[3][0]:.3f} ulp, cos {worst[3][1]:.3f} ulp; composites {ratio:.3f} of the bar")


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_non_finite_angle_poisons_exactly_its_constants(probe, bad):
    """NaN or +-inf in one angle: every constant that depends on that angle is NaN, every other one (C_X, C_Y, C_Z and
    those of the two finite angles) is finite and within its bar (branch 3: NaN raises the ballot)."""
    states = []
    for axis in range(3):
        for fin in (0.2, 0.6, 1.1):
            s = [fin, -fin, 0.5 * fin]
            s[axis] = bad
            states.append(tuple(s))
    rows = probe(states)
    for state, row in zip(states, rows):
        axis = "ypr"[[i for i in range(3) if not math.isfinite(state[i])][0]]
        assert tuple(row[:3]) == XYZ, (state, row[:3])
        sc = {}
        for k, a in zip("ypr", state):
            if math.isfinite(a):
                sc["s" + k], sc["c" + k] = exact_sincos(a)
        for name in NAMES[3:]:
            v = row[IDX[name]]
            if axis in DEPENDS[name]:
                assert math.isnan(v), (state, name, v)
                continue
            assert math.isfinite(v), (state, name, v)
            if name in COMPOSITES:
                val, bar = composite_exact_and_bar(name, sc, XYZ[0], ULP_BAR[3])
                assert abs(mpmath.mpf(v) - val) <= bar, (state, name)
            else:
                exact = {"T3": sc.get("sp"), "T24": sc.get("cp"), "CY": sc.get("cy"), "SY": sc.get("sy")}[name]
                assert ulp_error(v, exact) <= ULP_BAR[3], (state, name)
