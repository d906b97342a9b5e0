"""Deterministic inputs of tests/test_gpu_inverse_robust_edges.py (the robust inverse-compositional kernel's median scan
and its restated pixel loop), with what follows from them in closed form.  tests/test_inverse_robust_edges_cpu.py
holds every fixture to what the GPU file relies on, without a device.  The pixel-loop fixtures are tests/inverse_edges.py's,
the histogram's planes tests/inverse_robust_cases.py's.  Test infrastructure, not collected.

PLACED MEDIANS.  One 24x20 level under inverse_robust_cases.EDGE_K at the zero pose: every source pixel lands on its own
target pixel with weights exactly 0, so with I0 = 0 the residual of a row is its I1.  A placement is a list [(bin, count),
...]: `count` rows get I1 = (bin + 0.5) / 4096 -- exact in binary64, |r| * 4096 = bin + 0.5 exactly, the middle of the bin
-- at pixels drawn by a seeded permutation; the other pixels lose their depth (NaN) and are no rows.  Under
lambda_optimization_step = 0 the twist is -0 * step and Exp of it the identity, so the pose stays at zero bit for bit and
the entry pass and every iteration see the same residuals: for any iteration count the reported delta is scale * m and the
outliers are the rows with (bin + 0.5) / 4096 > delta, both from the list alone (placed_expect).  Thread t of the scan owns
bins 16 t ... 16 t + 15, wave w bins 1024 w ... 1024 w + 1023."""
import contextlib

import numpy as np

import inverse_edges as ie
import inverse_robust_cases as cases
import inverse_robust_ref as rr

N_PIXELS = cases.EDGE_W * cases.EDGE_H      # 480
PLACED_SEED = 11
PLACED_MAX_ITER = (1, 3)                  # 3: the reported delta comes from a histogram that was cleared twice and refilled
TIE_SCALE = 1.0
PLACED_SCALES = (rr.DEFAULT_SCALE, 0.5, TIE_SCALE)


def _mid(k):
    """The median inside bin k, with rows in the first thread's bins below it and in the last thread's above."""
    return [(7, 90), (k, 280), (4090, 110)]          # (half - before) / h[k] = 150 / 280: not the rows' own 0.5


def _placements():
    out = {}
    for w, t in enumerate((21, 85, 149, 213)):              # a thread inside each wave: its first and its last bin
        out[f"wave {w} thread {t} j=0"] = _mid(16 * t)
        out[f"wave {w} thread {t} j=15"] = _mid(16 * t + 15)
    # lane 63 of a wave and lane 0 of the next (bins 1008-1023 | 1024-1039, 2032-2047 | 2048-2063, 3056-3071 | 3072-3087),
    # and the two ends of the histogram
    out["wave 0 lane 0"] = [(2, 300), (4000, 180)]
    for k in (1010, 1030, 2040, 2050, 3060, 3080):
        out[f"wave {k // 1024} lane {(k // 16) % 64} bin {k}"] = _mid(k)
    out["wave 3 lane 63"] = [(7, 90), (4093, 390)]
    # the cumulative count meets `half` exactly at the end of a thread's last bin (this thread writes, not the next), of a
    # wave's last bin, each with the next bin adjacent and with empty bins in between (there the next thread's answer
    # would differ), and each beside its neighbour with one count moved across
    for name, k in (("thread 21", 16 * 21 + 15), ("thread 149", 16 * 149 + 15), ("wave 0", 1023), ("wave 1", 2047),
                    ("wave 2", 3071)):
        out[f"half at the end of {name}"] = [(k, 240), (k + 1, 240)]
        out[f"half at the end of {name}, one moved"] = [(k, 239), (k + 1, 241)]
        out[f"half at the end of {name}, then a gap"] = [(k, 240), (k + 600, 240)]
    out["below: every earlier wave"] = [(100, 50), (1500, 60), (2500, 70), (3500, 200), (3900, 100)]
    out["thread 85 j=2 and j=9"] = [(16 * 85 + 2, 200), (16 * 85 + 9, 280)]
    out["thread 149 j=2 and j=9 behind wave 0"] = [(50, 100), (16 * 149 + 2, 100), (16 * 149 + 9, 280)]
    out["n = 479"] = [(2047, 239), (2048, 240)]
    out["n = 451, wave 2"] = [(500, 101), (2600, 240), (3900, 110)]
    out["n = 1"] = [(1700, 1)]
    out["n = 2"] = [(900, 1), (2900, 1)]
    for k in (300, 1300, 2300, 3300):                       # every row in one bin: m is the rows' own value
        out[f"all in bin {k}"] = [(k, N_PIXELS)]
    for g in range(16):                                     # every swizzle group of hist_word holds a median once
        k = 64 * (g + 16 * (g % 4)) + 17 + g
        assert (k >> 6) & 15 == g and k // 1024 == g % 4
        out[f"swizzle group {g} bin {k}"] = _mid(k)
    out["tie"] = [(10, 140), (1500, 200), (3000, 140)]      # m = 1500.5 / 4096: the value of the 200 rows of bin 1500
    return out


PLACED = _placements()
PLACED_NAMES = tuple(PLACED)
# no gradient: with fewer than six rows H would be singular up to rounding only, and the two sides' pivots need not agree;
# with H exactly zero both meet an exact zero pivot (inverse_edges.rows_problem's constant source)
PLACED_NO_GRADIENT = ("n = 1", "n = 2")
# under TIE_SCALE these have |r| == delta exactly for the rows of the median's bin: they are inliers
PLACED_TIES = ("tie",) + tuple(f"all in bin {k}" for k in (300, 1300, 2300, 3300))


def placed_planes(name):
    """(i0, d0, gx0, gy0, i1) of a placement."""
    placement = PLACED[name]
    rs = np.random.RandomState(PLACED_SEED)
    gx0, gy0 = rs.uniform(-0.5, 0.5, (2, cases.EDGE_H, cases.EDGE_W))
    if name in PLACED_NO_GRADIENT:
        gx0, gy0 = np.zeros_like(gx0), np.zeros_like(gy0)
    perm = rs.permutation(N_PIXELS)
    i1, d0 = np.zeros(N_PIXELS), np.ones(N_PIXELS)
    at = 0
    for k, count in placement:
        i1[perm[at:at + count]] = (k + 0.5) / 4096.0
        at += count
    assert at <= N_PIXELS
    d0[perm[at:]] = np.nan
    shape = (cases.EDGE_H, cases.EDGE_W)
    return np.zeros(shape), d0.reshape(shape), gx0, gy0, i1.reshape(shape)


def placed_expect(placement, scale):
    """(rows, delta, outliers) of a placement by DESIGN.md §22's median rule, from the list alone."""
    placement = sorted(placement)
    n = sum(c for _, c in placement)
    half = (n + 1) // 2
    before = 0
    for k, count in placement:
        if before + count >= half:
            break
        before += count
    delta = scale * ((float(k) + float(half - before) / float(count)) * 2.0 ** -12)
    return n, delta, sum(c for b, c in placement if (b + 0.5) / 4096.0 > delta)


def placed_cfg(max_iter):
    return dict(num_levels=1, lam=[0.0], max_iter=[max_iter], min_grad=[0.0], min_depth=0.3, max_depth=5.0)


# ---- unit weights ----------------------------------------------------------------------------------------------------------
# A scale factor at which every weight of every fixture of this file is 1 (tests/test_inverse_robust_edges_cpu.py listens to
# every iteration): a power of two, so delta = UNIT_SCALE * m is exact.  m is at least 2^-13 wherever there is a row (half
# of the rows of bin 0 at the least), so delta is at least 2^27, beyond every finite intensity difference of these planes.
UNIT_SCALE = 2.0 ** 40


@contextlib.contextmanager
def weights_heard():
    """Listens to inverse_robust_ref.weights: yields a list that receives, per system, the number of weights that are
    not 1 (NaN residuals, which have no weight to speak of, left out).  inverse_robust_ref itself is not edited."""
    orig = rr.weights
    heard = []

    def listener(r, delta):
        w = orig(r, delta)
        heard.append(int(np.sum(w[np.isfinite(r)] != 1.0)))
        return w
    rr.weights = listener
    try:
        yield heard
    finally:
        rr.weights = orig


# ---- chunk counts ----------------------------------------------------------------------------------------------------------
# (w, h) -> chunks of 64 pixels per wave.  A wave that walks an odd number of chunks leaves the two-chunk pipeline at
# `!more1`, an even number at `!more0`; the parity sizes of inverse_robust_cases give wave 0 only 1, 2 or 16.
CHUNK_SIZES = {(24, 24): [3, 2, 2, 2], (28, 27): [3, 3, 3, 3], (26, 32): [4, 3, 3, 3], (12, 10): [1, 1, 0, 0]}
CHUNK_MAX_ITER = [5]
CHUNK_SEARCH = range(1, 30)               # tests/test_inverse_robust_edges_cpu.py searches these seeds again
CHUNK_SEED = {(24, 24): 1, (28, 27): 1, (26, 32): 1, (12, 10): 1}


def chunks_per_wave(w, h):
    n = -(-(w * h) // 64)
    return [len(range(wave, n, 4)) for wave in range(4)]


def chunk_pair(w, h):
    return cases.small_pair(CHUNK_SEED[(w, h)], w, h)


def final_rotation(pyr, K, config):
    """inverse_edges.final_rotation for the robust checker: (its record, the rotation matrix its last level ended with)."""
    orig = rr.ir.state_from_pose
    seen = []

    def listener(R, t):
        seen.append(np.array(R))
        return orig(R, t)
    rr.ir.state_from_pose = listener
    try:
        ref = rr.optimize(pyr, K, config)
    finally:
        rr.ir.state_from_pose = orig
    return ref, seen[-1]


# ---- the footing of a pixel-loop fixture under objective 6 -------------------------------------------------------------
def footing(ref):
    """What the exact counts of a comparison with inverse_robust_ref.optimize rest on: the reasons this result has none."""
    why = []
    if not ref["margin"] > ie.MARGIN_FLOOR:
        why.append(f"gradient threshold margin {ref['margin']:.3e}")
    if not ref["bin_margin"] >= cases.BIN_MARGIN_FLOOR:
        why.append(f"bin margin {ref['bin_margin']:.3e}")
    if not ref["delta_margin"] >= cases.DELTA_MARGIN_FLOOR:
        why.append(f"delta margin {ref['delta_margin']:.3e}")
    return why
