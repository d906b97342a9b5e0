"""The order of the normal-equation sums (csrc/gn_device.hpp: wave_butterfly, reduce_wave_to_row, sum_rows_broadcast), bit for bit.

Every Gauss-Newton kernel folds 27 sums and a row count over the lanes of a wave and the waves of a workgroup in one fixed
order, whatever the values travel through (lane swaps, DPP moves, LDS).  tests/native/reduction_probe.hip runs the header's
functions unchanged on per-lane accumulators given by the caller, for workgroups of 1, 4, 8 and 16 waves; this file holds
the 28 totals it returns to a numpy float64 emulation of the documented order, written out below:

  per wave   a transposed butterfly over the 64 lanes, 32 values per lane.  Stage d = 32, 16, 8, 4, 2 halves the N = 32, 16,
             8, 4, 2 values a lane still holds: with p = lane ^ d, a lane whose bit d is clear takes
             v[i] = v[i] + p.v[i], a lane whose bit is set v[i] = v[i + N/2] + p.v[i + N/2] (i < N/2); stage d = 1 adds the
             last value of the two lanes of a pair.  Lane l ends with the wave's sum of value
             idx(l) = 16 b5 + 8 b4 + 4 b3 + 2 b2 + b1 (b_k = bit k of l), which the even lane stores in the wave's row.
  per group  value j of the rows of the first half of the waves is added row by row to 0.0, the same for the second half,
             and the total is first + second.  A single wave's row is the total itself.

fp64 addition is commutative bit for bit except for the payload of a NaN, so "keep + received" and "received + keep" are one
order here, and a NaN is compared as a NaN.  The first test needs no GPU: it shows that the random inputs tell this order from
another one, without which the comparison on the device could not fail.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")

WAVE, NRED, TOTALS, RED_VALID = 64, 32, 28, 27
WAVES = [1, 4, 8, 16]
LANES = np.arange(WAVE)
# value index a lane ends with
IDX = ((LANES >> 5) & 1) * 16 + ((LANES >> 4) & 1) * 8 + ((LANES >> 3) & 1) * 4 + ((LANES >> 2) & 1) * 2 + ((LANES >> 1) & 1)


# ------------------------------------------------------------------------------------------------------------------------
# the documented order, in numpy float64 (IEEE additions, subnormals kept: what the device does in fp64)
# ------------------------------------------------------------------------------------------------------------------------
def wave_row(v):
    """v: [64 lanes, 32 values] of one wave -> its row of 32 sums."""
    v = np.array(v, dtype=np.float64)
    n = NRED
    with np.errstate(all="ignore"):
        for d in (32, 16, 8, 4, 2):
            p = v[LANES ^ d]
            bit_set = ((LANES & d) != 0)[:, None]
            low = v[:, :n // 2] + p[:, :n // 2]                 # bit clear: keeps v[i], receives the partner's v[i]
            high = v[:, n // 2:n] + p[:, n // 2:n]              # bit set: keeps v[i + N/2], receives the partner's
            v = np.where(bit_set, high, low)
            n //= 2
        total = v[:, 0] + v[LANES ^ 1, 0]
    row = np.zeros(NRED)
    even = LANES[(LANES & 1) == 0]
    row[IDX[even]] = total[even]
    return row


def documented_totals(acc):
    """acc: [waves, 64, 32] -> the 28 totals of the workgroup."""
    rows = np.stack([wave_row(w) for w in acc])
    nw = rows.shape[0]
    if nw == 1:
        return rows[0, :TOTALS].copy()
    with np.errstate(all="ignore"):
        first = np.zeros(NRED)
        for w in range(nw // 2):
            first = first + rows[w]
        second = np.zeros(NRED)
        for w in range(nw // 2, nw):
            second = second + rows[w]
        return (first + second)[:TOTALS]


def sequential_totals(acc):
    """Another order: lane after lane, wave after wave."""
    flat = np.asarray(acc, dtype=np.float64).reshape(-1, NRED)
    out = np.zeros(NRED)
    with np.errstate(all="ignore"):
        for r in flat:
            out = out + r
    return out[:TOTALS]


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
# decimal exponent ranges of the random cases: nearly the full span of fp64, and narrower ones, where many terms of a sum
# share their leading bits (the sums of a real alignment look like those)
SPANS = [(-300, 300), (-300, 300), (-12, 12), (-2, 2), (-300, -285), (285, 300)]


def random_cases(waves):
    rng = np.random.default_rng(20260 + waves)
    out = []
    for lo, hi in SPANS:
        mag = 10.0 ** rng.uniform(lo, hi, size=(waves, WAVE, NRED))
        sign = np.where(rng.random((waves, WAVE, NRED)) < 0.5, -1.0, 1.0)
        out.append(mag * sign)
    return out


def special_cases(waves):
    """name -> accumulators.  Slots 28..31 are padding: whatever they hold must not reach a total."""
    rng = np.random.default_rng(977 + waves)
    n = waves * WAVE
    cases = {}
    # exact cancellations: every value has its negative somewhere else in the workgroup, in another order per slot
    half = 10.0 ** rng.uniform(-20, 20, size=(n // 2, NRED))
    both = np.concatenate([half, -half])
    cases["cancellations"] = np.stack([both[rng.permutation(n), j] for j in range(NRED)], axis=1).reshape(waves, WAVE, NRED)
    # signed zeros: all -0 (a single wave's total stays -0; 0.0 + -0 is +0 once rows are summed), all +0, and a mix
    cases["minus_zero"] = np.full((waves, WAVE, NRED), -0.0)
    cases["plus_zero"] = np.zeros((waves, WAVE, NRED))
    cases["mixed_zero"] = np.where(rng.random((waves, WAVE, NRED)) < 0.5, -0.0, 0.0)
    # subnormals only, and subnormals next to the smallest normals
    sub = rng.integers(1, 1 << 40, size=(waves, WAVE, NRED)).astype(np.float64) * 5e-324
    cases["subnormals"] = sub * np.where(rng.random(sub.shape) < 0.5, -1.0, 1.0)
    cases["subnormal_edge"] = cases["subnormals"] + np.where(rng.random(sub.shape) < 0.1, 2.2250738585072014e-308, 0.0)
    # one +inf in slot 3, one -inf in slot 5, both in slot 7 (NaN), at lanes of different waves
    inf = 10.0 ** rng.uniform(-3, 3, size=(waves, WAVE, NRED))
    inf[0, 5, 3] = math.inf
    inf[waves - 1, 62, 5] = -math.inf
    inf[0, 17, 7] = math.inf
    inf[waves - 1, 40, 7] = -math.inf
    cases["infinities"] = inf
    # one NaN in slot 11: that total is NaN, every other one is untouched; and a NaN in the padding, which reaches nothing
    nan = 10.0 ** rng.uniform(-3, 3, size=(waves, WAVE, NRED))
    nan[waves // 2, 33, 11] = math.nan
    nan[0, 9, 30] = math.nan
    cases["nan"] = nan
    # row counts as the kernels put them in: an integer per lane in the spare slot
    counts = 10.0 ** rng.uniform(-3, 3, size=(waves, WAVE, NRED))
    counts[:, :, RED_VALID] = rng.integers(0, 65, size=(waves, WAVE)).astype(np.float64)
    cases["row_counts"] = counts
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the emulation itself, and whether the inputs can tell one order from another
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", WAVES)
def test_random_cases_are_order_sensitive(waves):
    """For at least half of the random cases another order of the same additions (lane after lane, wave after wave) gives
    different bits than the documented one.  math.fsum, the correctly rounded sum, bounds the emulation: the documented
    order stays within the rounding of its additions of it."""
    cases = random_cases(waves)
    sensitive = 0
    for acc in cases:
        doc, seq = documented_totals(acc), sequential_totals(acc)
        differ = ~same_bits(doc, seq)
        if differ.any():
            sensitive += 1
        flat = acc.reshape(-1, NRED)
        exact = np.array([math.fsum(flat[:, j]) for j in range(TOTALS)])
        # both orders are orders of the same sum: within a few ulp of the sum of magnitudes of the exact one
        scale = np.array([math.fsum(np.abs(flat[:, j])) for j in range(TOTALS)])
        assert np.all(np.abs(doc - exact) <= flat.shape[0] * 2.0 ** -52 * scale)
    assert 2 * sensitive >= len(cases), (sensitive, len(cases))


def test_emulation_on_known_sums():
    """Integers sum exactly in any order: the emulation returns their sum in every slot, from the right lanes' values."""
    for waves in WAVES:
        acc = np.zeros((waves, WAVE, NRED))
        for j in range(NRED):
            acc[:, :, j] = (np.arange(waves * WAVE).reshape(waves, WAVE) % 7) * (j + 1)
        expect = acc.sum(axis=(0, 1))[:TOTALS]
        assert np.array_equal(documented_totals(acc), expect)
    one = np.full((1, WAVE, NRED), -0.0)
    assert np.all(np.signbit(documented_totals(one)))                     # a single wave: -0 survives
    four = np.full((4, WAVE, NRED), -0.0)
    assert not np.any(np.signbit(documented_totals(four)))                # rows are added to +0.0


def test_one_wave_kernel_is_pinned():
    """The one-wave-per-pair level kernel (64 threads) starts on a 4 KB boundary and opens with a pad of 896 s_nop in every
    plane storage, so that its loops lie where they were measured whatever else the code object holds (csrc/gn_kernels.hip,
    gn_level_kernel); the kernels of more waves keep the default alignment and carry no pad."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "isa-level"])
    text = open(os.path.join(CSRC, "build", "gn_kernels.s")).read()
    bodies = {}
    for m in re.finditer(r"^(_ZN9phovo_hip\S*gn_level_kernelILi(\d+)E\S*):", text, re.M):
        end = text.index(".Lfunc_end", m.end())
        head = text[max(0, m.start() - 400):m.start()]
        bodies[m.group(1)] = (int(m.group(2)), re.findall(r"\.p2align\s+(\d+)", head)[-1], text[m.end():end])
    one_wave = [v for v in bodies.values() if v[0] == 64]
    assert len(one_wave) == 3 and len(bodies) > 3
    for threads, align, body in bodies.values():
        fills = re.findall(r"\.fill\s+(\d+), 4, 0xbf800000", body)
        assert (align, fills) == (("12", ["896"]) if threads == 64 else ("8", [])), (threads, align, fills)


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def build_probe():
    subprocess.check_call(["make", "-s", "-C", CSRC, "reduction-probe"])
    return os.path.join(CSRC, "build", "reduction_probe.so")


@pytest.fixture(scope="module")
def probe():
    lib = ctypes.CDLL(build_probe())
    lib.reduction_probe_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.reduction_probe_values_per_lane() == NRED and lib.reduction_probe_totals() == TOTALS

    def run(cases, waves):
        data = np.ascontiguousarray(np.stack(cases), dtype=np.float64)
        assert data.shape == (len(cases), waves, WAVE, NRED)
        out = np.full((len(cases), 2, TOTALS), 12345.0)
        n_valid = np.full((len(cases), 2), -7, dtype=np.int32)
        status = lib.reduction_probe_run(data.ctypes.data, len(cases), waves, out.ctypes.data, n_valid.ctypes.data)
        assert status == 0, status
        return out, n_valid
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_device_totals_follow_the_documented_order(probe, waves):
    """Random magnitudes over 1e-300 .. 1e300 and narrower spans, mixed signs: the 28 totals equal the emulation's bit for
    bit, in lane 0 and in lane 63 of the wave that sums the rows."""
    cases = random_cases(waves)
    out, _ = probe(cases, waves)
    for c, acc in enumerate(cases):
        expect = documented_totals(acc)
        for which in (0, 1):
            ok = same_bits(out[c, which], expect)
            assert ok.all(), (waves, c, which, np.flatnonzero(~ok), out[c, which][~ok], expect[~ok])


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_device_totals_on_special_values(probe, waves):
    """Exact cancellations, signed zeros, subnormals, +-inf (and inf - inf), NaN in a sum and in the padding, row counts."""
    cases = special_cases(waves)
    names = list(cases)
    out, n_valid = probe([cases[k] for k in names], waves)
    for c, name in enumerate(names):
        expect = documented_totals(cases[name])
        for which in (0, 1):
            ok = same_bits(out[c, which], expect)
            assert ok.all(), (waves, name, which, np.flatnonzero(~ok), out[c, which][~ok], expect[~ok])
    i = names.index("minus_zero")
    assert np.all(np.signbit(out[i, 0]) == (waves == 1))
    i = names.index("infinities")
    assert out[i, 0, 3] == math.inf and out[i, 0, 5] == -math.inf and math.isnan(out[i, 0, 7])
    assert np.isfinite(np.delete(out[i, 0], [3, 5, 7])).all()
    i = names.index("nan")
    assert math.isnan(out[i, 0, 11]) and np.isfinite(np.delete(out[i, 0], 11)).all()
    i = names.index("row_counts")
    assert n_valid[i, 0] == n_valid[i, 1] == int(cases["row_counts"][:, :, RED_VALID].sum())

