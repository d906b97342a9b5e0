"""The arithmetic helpers of csrc/gn_device.hpp on the device, each against an exact or high-precision reference.

tests/native/arith_probe.hip includes the header unchanged and runs fast_rcp<1|2>, round_half_up_from, rowcol_from_index /
_floor, rowcol_advance, mad24_uniform_b, plane_load<double|float|__half> (through plane_rsrc and frame_rsrc), solve6_ldlt,
solve6_cholesky and solve8_ldlt on plain arrays, one thread per element.  The inputs and references live in
tests/device_arith.py; tests/test_device_arith_cpu.py checks them without a GPU.  Each test prints the worst figure it
measured before it asserts (DESIGN.md §4 keeps the table).
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import device_arith as da

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")
GROUP = 64


def build_probe():
    subprocess.check_call(["make", "-s", "-C", CSRC, "arith-probe"])
    return os.path.join(CSRC, "build", "arith_probe.so")


class Probe:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.guard = self.lib.arith_probe_guard_bytes()
        self.sentinel = self.lib.arith_probe_sentinel()

    @staticmethod
    def _p(a):
        return ctypes.c_void_p(a.ctypes.data)

    def rcp(self, x, steps):
        x = np.ascontiguousarray(x, dtype=np.float64)
        r = np.full(x.size, 12345.0)
        assert self.lib.arith_probe_rcp(self._p(x), x.size, steps, self._p(r)) == 0
        return r

    def round_half(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = np.full(v.size, 12345.0)
        assert self.lib.arith_probe_round_half(self._p(v), v.size, self._p(out)) == 0
        return out

    def rowcol(self, W, k, floor_form):
        """(W[i], k[i]) in any order: grouped by width into 64-thread workgroups (padded with k = 0) for the probe."""
        W = np.asarray(W, dtype=np.int64)
        k = np.asarray(k, dtype=np.int64)
        order = np.argsort(W, kind="stable")
        Ws, ks = W[order], k[order]
        widths, first, count = np.unique(Ws, return_index=True, return_counts=True)
        groups = (count + GROUP - 1) // GROUP
        slot0 = np.concatenate([[0], np.cumsum(groups)[:-1]]) * GROUP            # first slot of every width
        slot = np.repeat(slot0 - first, count) + np.arange(Ws.size)
        n = int(groups.sum()) * GROUP
        kk = np.zeros(n, dtype=np.int32)
        kk[slot] = ks
        wg = np.repeat(widths, groups).astype(np.int32)
        c = np.full(n, 12345.0)
        r = np.full(n, 12345.0)
        assert self.lib.arith_probe_rowcol(self._p(kk), n, self._p(wg), int(floor_form), self._p(c), self._p(r)) == 0
        cc = np.empty(W.size)
        rr = np.empty(W.size)
        cc[order], rr[order] = c[slot], r[slot]
        return cc, rr

    def rowcol_walk(self, walks):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        W, start, sr, sc, steps = (i32(walks[q]) for q in ("W", "start", "step_r", "step_c", "steps"))
        off = np.concatenate([[0], np.cumsum(walks["steps"])[:-1]]).astype(np.int64)
        total = int(walks["steps"].sum())
        c = np.full(total, 12345.0)
        r = np.full(total, 12345.0)
        status = self.lib.arith_probe_rowcol_walk(W.size, self._p(W), self._p(start), self._p(sr), self._p(sc), self._p(steps),
                                                  self._p(off), ctypes.c_longlong(total), self._p(c), self._p(r))
        assert status == 0
        return off, c, r

    def mad24(self, a, b, c):
        a = np.ascontiguousarray(a, dtype=np.int32)
        c = np.ascontiguousarray(c, dtype=np.int32)
        out = np.full(a.size, -7, dtype=np.int32)
        assert self.lib.arith_probe_mad24(self._p(a), int(b), self._p(c), a.size, self._p(out)) == 0
        return out

    def load(self, storage, payload, num_records, soff, idx):
        payload = np.ascontiguousarray(payload).view(np.uint8)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.full(idx.size, 12345.0)
        status = self.lib.arith_probe_load(storage, self._p(payload), payload.size, int(num_records), int(soff), self._p(idx),
                                           idx.size, self._p(out))
        assert status == 0, status
        return out

    def solve(self, which, h, g):
        h = np.ascontiguousarray(h, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        x = np.full(g.shape, 12345.0)
        fn = self.lib.arith_probe_solve6 if which == 6 else self.lib.arith_probe_solve8
        assert h.shape == (g.shape[0], which * (which + 1) // 2) and g.shape[1] == which
        assert fn(self._p(h), self._p(g), g.shape[0], self._p(x)) == 0
        return x

    def solve6_chol(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert a.shape == (b.shape[0], 21) and b.shape[1] == 6
        y = np.full(b.shape, 12345.0)
        ok = np.full(b.shape[0], -7, dtype=np.int32)
        assert self.lib.arith_probe_solve6_chol(self._p(a), self._p(b), b.shape[0], self._p(y), self._p(ok)) == 0
        return y, ok


@pytest.fixture(scope="module")
def probe():
    return Probe(build_probe())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------
# fast_rcp
# ------------------------------------------------------------------------------------------------------------------------
def test_fast_rcp_two_steps_is_within_one_ulp(probe):
    """fast_rcp<2>: at most one ulp from the correctly rounded 1 / x (numpy's IEEE division) for 2^-1000 <= |x| <= 2^1000."""
    worst = 0
    for name, x in da.rcp_inputs().items():
        r = probe.rcp(x, 2)
        d = da.ulp_distance(r, 1.0 / x)
        i = int(d.argmax())
        print(f"fast_rcp<2> {name}: {x.size} values, worst {int(d[i])} ulp at x = {x[i]!r} ({x[i].hex()}), "
              f"{np.count_nonzero(d)} not correctly rounded")
        worst = max(worst, int(d[i]))
        assert np.all(np.signbit(r) == np.signbit(x))
    assert worst <= 1


def test_fast_rcp_one_step_is_within_2_to_the_minus_48(probe):
    """fast_rcp<1>: relative error at most 2^-48 (the figure at its call site in gn_kernels.hip), exactly: an error of d ulp
    of the correctly rounded quotient is a relative error below (d + 1/2) 2^-52, which settles every value with d <= 15;
    the rest, and the worst 200 of each set, are measured in rational arithmetic."""
    worst = 0
    for name, x in da.rcp_inputs().items():
        r = probe.rcp(x, 1)
        d = da.ulp_distance(r, 1.0 / x)
        assert np.all(np.signbit(r) == np.signbit(x)) and np.all(np.isfinite(r))
        check = np.union1d(np.flatnonzero(d > 15), np.argsort(d)[-200:])
        errs = [(da.rcp_relative_error(x[i], r[i]), i) for i in check]
        e, i = max(errs)
        print(f"fast_rcp<1> {name}: {x.size} values, worst {int(d.max())} ulp, worst relative error 2^{math.log2(float(e)):.2f} "
              f"at x = {x[i]!r} ({x[i].hex()})")
        worst = max(worst, e)
    assert worst <= 2.0 ** -48


# What fast_rcp returns where 1 / x is not a finite non-zero number: the seed is the IEEE quotient (v_rcp_f64 gives +-inf
# for +-0 and +-0 for +-inf) and the first Newton step forms 0 x inf, so every such input gives NaN.
def test_fast_rcp_special_inputs_give_the_quotient_or_nan(probe):
    x = np.array([0.0, -0.0, math.inf, -math.inf, math.nan])
    with np.errstate(all="ignore"):
        quotient = 1.0 / x
    for steps in (1, 2):
        r = probe.rcp(x, steps)
        print(f"fast_rcp<{steps}> of {x.tolist()}: {r.tolist()}")
        assert np.all(np.isnan(r) | (bits(r) == bits(quotient)))          # never a finite wrong number
        assert np.all(np.isnan(r))                                         # which it is: NaN, for all five


# ------------------------------------------------------------------------------------------------------------------------
# round_half_up_from
# ------------------------------------------------------------------------------------------------------------------------
def test_round_half_up_from_is_c_round_on_the_whole_table(probe):
    """The candidate table of tests/test_oracle_properties.py through the device's two instructions: C round() exactly,
    +0 (never -0, never a value below 0) for everything in (-0.5, 0.5)."""
    v, expect = da.round_table()
    out = probe.round_half(v)
    bad = np.flatnonzero(bits(out) != bits(expect + 0.0))
    print(f"round_half_up_from: {v.size} values, {bad.size} wrong" + (f", first {v[bad[0]]!r} -> {out[bad[0]]!r}" if bad.size else ""))
    assert bad.size == 0
    assert not np.any(np.signbit(out))


# ------------------------------------------------------------------------------------------------------------------------
# rowcol_from_index, rowcol_from_index_floor, rowcol_advance
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor_form", [False, True])
def test_rowcol_from_index_is_divmod(probe, floor_form):
    sets = [("boundary", da.rowcol_boundary_points()), ("random", da.rowcol_random_points())]
    if floor_form:
        sets.append(("negative", da.rowcol_negative_points()))
    for name, (W, k) in sets:
        c, r = probe.rowcol(W, k, floor_form)
        er, ec = np.divmod(k, W)                              # numpy's integer divmod floors, as Python's
        bad = np.flatnonzero((c != ec) | (r != er))
        print(f"rowcol_from_index{'_floor' if floor_form else ''} {name}: {W.size} points, {bad.size} wrong" +
              (f", first W = {W[bad[0]]}, k = {k[bad[0]]}: ({c[bad[0]]}, {r[bad[0]]})" if bad.size else ""))
        assert bad.size == 0
        assert not np.any(np.signbit(c))                      # an integer-valued double, +0 at the row start


def test_rowcol_advance_walks_a_whole_level(probe):
    """Every step of the chunk walk equals divmod(start + i threads, W), for the first and the last lane of workgroups of
    64 .. 1024 threads, widths below and above the workgroup size."""
    w = da.rowcol_walks()
    assert np.all(w["step_c"] < w["W"])                       # the single-wrap precondition, on the inputs themselves
    off, c, r = probe.rowcol_walk(w)
    wrong = 0
    for i in range(len(w["W"])):
        steps = int(w["steps"][i])
        k = w["start"][i] + np.arange(1, steps + 1, dtype=np.int64) * w["threads"][i]
        er, ec = np.divmod(k, w["W"][i])
        sl = slice(int(off[i]), int(off[i]) + steps)
        bad = np.flatnonzero((c[sl] != ec) | (r[sl] != er))
        if bad.size:
            print(f"walk W = {w['W'][i]}, threads = {w['threads'][i]}, start = {w['start'][i]}: first wrong step {bad[0] + 1}")
        wrong += bad.size
    print(f"rowcol_advance: {len(w['W'])} walks, {int(w['steps'].sum())} steps, {wrong} wrong")
    assert wrong == 0


# ------------------------------------------------------------------------------------------------------------------------
# mad24_uniform_b
# ------------------------------------------------------------------------------------------------------------------------
def test_mad24_is_the_32_bit_multiply_add(probe):
    """a * b + c in 32-bit integers: corners and random values of [0, 2^21]^3 below 2^31, the kernels' row * W + column at
    the edges of H * W <= 2^21, and one documented row each at the limits of the instruction's 24-bit signed operand,
    a = 2^23 - 1 and a = -1, where it is still exact."""
    total = 0
    for b, a, c, note in da.mad24_cases():
        out = probe.mad24(a, b, c)
        expect = (a * b + c).astype(np.int32)
        assert np.array_equal(out, expect), (note, b, a[out != expect][:4], c[out != expect][:4], out[out != expect][:4])
        total += a.size
    print(f"mad24_uniform_b: {total} values exact")


# ------------------------------------------------------------------------------------------------------------------------
# plane_load
# ------------------------------------------------------------------------------------------------------------------------
def same_or_nan(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("storage", [0, 1, 2])
def test_plane_load_widens_exactly_and_reads_zero_outside_the_plane(probe, storage):
    """plane_rsrc: every element widens to the fp64 numpy gives (subnormals kept, +-0, +-inf, NaN as NaN), and idx = -1,
    idx = n and beyond read +0.0 -- also when the next plane's data, not the guard, lies behind the n-th element."""
    plane = da.load_plane(storage)
    n, size = plane.size, plane.dtype.itemsize
    idx = np.concatenate([np.arange(n), [-1, n, n + 1, n + 1000]])
    expect = np.concatenate([plane.astype(np.float64), [0.0] * 4])
    for payload in (plane, np.concatenate([plane, plane[::-1]])):
        out = probe.load(storage, payload, n * size, 0, idx)
        ok = same_or_nan(out, expect)
        assert ok.all(), (storage, idx[~ok][:5], out[~ok][:5], expect[~ok][:5])
    sub = (plane != 0) & (np.abs(plane.astype(np.float64)) < np.finfo(plane.dtype).tiny)
    assert np.count_nonzero(out[:n][sub] != 0) == np.count_nonzero(sub) > 2000                 # no subnormal flushed


@pytest.mark.parametrize("storage", [0, 1, 2])
def test_frame_descriptor_range_check_includes_the_scalar_offset(probe, storage):
    """frame_rsrc + soff: one descriptor over a "frame" of three planes, soff = the plane's byte offset.  In-plane reads
    are exact.  The range check includes the scalar offset: a read is served iff
    soff + idx * size + size <= num_records, so
      * a read whose address lies behind the frame reads +0.0, whichever of soff and idx carries it there, and so does
        idx = -1 with any soff: nothing behind (or in front of) the frame is ever read;
      * a read past plane p that is still inside the frame returns the element of the plane that lies there, NOT 0: "past
        the plane reads 0" holds for a per-plane descriptor (plane_rsrc) only.  No kernel uses such a value: every read
        past a plane through a frame descriptor belongs to a lane that is masked out (DESIGN.md §4 lists them)."""
    whole = da.load_plane(storage)
    plane = np.concatenate([whole[:512], whole[-500:]])        # specials, subnormals, ordinary values: at most 8 KB, so that
    n, size = plane.size, plane.dtype.itemsize                 # two planes past the frame still lie inside the probe's guard
    assert 2 * n * size + 64 <= probe.guard
    frame = np.concatenate([np.roll(plane, 7), plane, np.roll(plane, 13)])
    wide = frame.astype(np.float64).reshape(3, n)
    records = 3 * n * size
    past = np.arange(10)
    for p in range(3):
        soff = p * n * size
        out = probe.load(storage, frame, records, soff, np.arange(n))
        assert same_or_nan(out, wide[p]).all(), (storage, p)
        out = probe.load(storage, frame, records, soff, np.concatenate([[-1], 3 * n + past]))
        assert np.all(bits(out) == 0), (storage, p, out)
        for q in range(1, 3):                                  # q planes further on
            out = probe.load(storage, frame, records, soff, q * n + past)
            inside = p + q < 3
            print(f"storage {storage}: plane {p}, idx = {q}n .. : {'inside the frame' if inside else 'behind the frame'}: "
                  f"{out[:3].tolist()}")
            if inside:
                assert same_or_nan(out, wide[p + q][past]).all(), (storage, p, q, out)
            else:
                assert np.all(bits(out) == 0), (storage, p, q, out)
    # the last element of the frame is readable through every plane's offset, the one behind it through none
    for p in range(3):
        out = probe.load(storage, frame, records, p * n * size, np.array([(3 - p) * n - 1, (3 - p) * n]))
        assert same_or_nan(out[:1], wide[2][-1:]).all() and bits(out)[1] == 0, (storage, p, out)


# ------------------------------------------------------------------------------------------------------------------------
# the solvers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["n6", "n8", "chol"])
def test_solver_is_accurate_to_cond_eps(probe, kind):
    """|x - x_exact|_2 <= c cond2(H) 2^-53 |x_exact|_2 per system, x_exact from mpmath at 400 bits, c four times the worst
    factor of the reference's own method on the same draws (tests/device_arith.py, REFERENCE_FACTOR)."""
    n = 8 if kind == "n8" else 6
    h, g = da.solver_systems(kind)
    if kind == "chol":
        x, ok = probe.solve6_chol(h, g)
        assert np.all(ok == 1)                                 # true for every positive definite system
    else:
        x = probe.solve(n, h, g)
    assert np.all(np.isfinite(x))
    frac = da.error_fraction(x, kind)
    nrand = da.random_spd(n)[0].shape[0]
    cond = da.exact_solutions(kind)[1]
    i = int(frac.argmax())
    print(f"{kind}: {len(frac)} systems ({len(frac) - nrand} real), c = {da.bar_factor(n):.3f}, worst fraction of the bar "
          f"{frac.max() / da.bar_factor(n):.3f} (system {i}, cond {cond[i]:.3g}); real systems alone "
          f"{frac[nrand:].max() / da.bar_factor(n):.3f}")
    assert np.all(frac <= da.bar_factor(n)), (i, frac[i])


@pytest.mark.parametrize("n", [6, 8])
def test_ldlt_returns_a_non_finite_component_on_a_singular_system(probe, n):
    """Rank n - 1 with an exact zero pivot: at least one component of x is not finite (the kernels turn that into
    PHOVO_PAIR_NONFINITE)."""
    h, g, _ = da.singular_systems(n)
    x = probe.solve(n, h, g)
    assert np.all(~np.isfinite(x).all(axis=1)), x


def test_cholesky_says_no_to_what_is_not_positive_definite(probe):
    """False for an exactly singular system, a negative pivot, a NaN entry and an infinite diagonal (at every position: an
    infinite LAST pivot is caught by the finiteness test alone)."""
    hs, gs, _ = da.singular_systems(6)
    h, g, _ = da.random_spd(6)
    H = da.full(h[3], 6)
    bad = [da.full(q, 6) for q in hs]
    rhs = list(gs)
    neg = H.copy(); neg[2, 2] = -neg[2, 2]; bad.append(neg)
    ind = H.copy(); ind[0, 1] = ind[1, 0] = 2.0 * math.sqrt(H[0, 0] * H[1, 1]); bad.append(ind)      # negative second pivot
    nan = H.copy(); nan[0, 3] = nan[3, 0] = math.nan; bad.append(nan)
    nand = H.copy(); nand[5, 5] = math.nan; bad.append(nand)
    for j in range(6):
        inf = H.copy(); inf[j, j] = math.inf; bad.append(inf)
    rhs += [g[3]] * (len(bad) - len(rhs))
    _, ok = probe.solve6_chol(np.array([da.upper(b) for b in bad]), np.array(rhs))
    assert np.all(ok == 0), ok
