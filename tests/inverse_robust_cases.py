"""Fixtures of the robust inverse-compositional objective (PHOVO_OBJECTIVE_INVERSE_ROBUST), shared by
tests/test_inverse_robust_cpu.py (which checks that they keep away from the places where rounding could move a count) and
tests/test_gpu_inverse_robust.py (which runs them on the device).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic

# every |r| * 4096 stays this far (in bins) from the integers 1, 2, ..., and every |r| this far from its delta
BIN_MARGIN_FLOOR = 1e-7
DELTA_MARGIN_FLOOR = 1e-10


def occluder(gray1, seed, f):
    """gray1 with a textured rectangle covering the share f of the image painted in (f = 0: a copy)."""
    out = gray1.copy()
    if f <= 0:
        return out
    h, w = gray1.shape
    rs = np.random.RandomState(100 + seed)
    hh, ww = int(h * np.sqrt(f)), int(w * np.sqrt(f))
    r0, c0 = rs.randint(0, h - hh), rs.randint(0, w - ww)
    x, y = np.meshgrid(np.arange(ww, dtype=np.float64), np.arange(hh, dtype=np.float64))
    out[r0:r0 + hh, c0:c0 + ww] = (127 + 100 * np.sin(x / 3 + seed) * np.cos(y / 4)).astype(np.uint8)
    return out


def occluded_pair(seed, f, w=160, h=120):
    p = synthetic.make_pair(seed, w, h)
    p["gray1"] = occluder(p["gray1"], seed, f)
    return p


def small_pair(seed, w, h):
    return synthetic.make_pair(seed, w, h, holes=0.02, trans=0.01, rot=0.005)


# name -> (pair, levels, max_iter, min_grad): the parity fixtures.  The seeds are the first that pass the pre-checks of
# tests/test_inverse_robust_cpu.py (conditioning, threshold margin, bin and delta margins); of the accuracy test's seeds
# 1 .. 5 under the occluder, 1 .. 4 come within 1e-7 bins of a bin's edge (3 and 4 sit exactly on one) and 5 does not.
PARITY = {
    "8x8": (lambda: small_pair(1, 8, 8), 1, [5], [0.0]),
    "7x5": (lambda: small_pair(1, 7, 5), 1, [5], [0.0]),
    "20x16": (lambda: small_pair(1, 20, 16), 1, [5], [0.0]),
    "75x53": (lambda: small_pair(1, 75, 53), 1, [5], [0.0]),
    "24x20 two levels": (lambda: small_pair(1, 24, 20), 2, [5, 5], [0.0, 0.0]),
    "160x120 occluded": (lambda: occluded_pair(5, 0.1), 3, [10, 10, 10], [0.0] * 3),
}
# the work queue's and the bit-identity test's pairs (24x20 two levels; 80x60 two levels with a gradient threshold)
QUEUE_SEEDS = (1, 2, 3)
IDENTITY = (lambda: synthetic.make_pair(5, 80, 60, holes=0.02), lambda: synthetic.make_pair(6, 80, 60, holes=0.02),
            2, [6, 6], [5.0, 5.0])
SCALE_PAIR = (lambda: occluded_pair(2, 0.1, 80, 60), 2, [8, 8], [0.0, 0.0])


# ---- histogram edges: 24 x 20, planes set plane by plane -------------------------------------------------------------------
EDGE_W, EDGE_H = 24, 20
# fx = fy = 32, integer principal point, depth 1: at zero motion every source pixel lands on its own target pixel with
# weights exactly 0, so r = I1 - I0 exactly
EDGE_K = np.array([[32.0, 0.0, 12.0], [0.0, 32.0, 10.0], [0.0, 0.0, 1.0]])


def edge_planes(kind):
    """(source planes (i0, d0, gx0, gy0), target intensity i1) of one histogram-edge case, and what the median rule must give:
    (m, outliers under the default scale factor), None where the case states no closed form."""
    n = EDGE_W * EDGE_H
    rs = np.random.RandomState(7)
    d0 = np.ones((EDGE_H, EDGE_W))
    gx0, gy0 = rs.uniform(-0.5, 0.5, (2, EDGE_H, EDGE_W))
    i0 = np.zeros((EDGE_H, EDGE_W))
    half = (n + 1) // 2
    if kind == "equal":                                   # bin 0
        i0 = rs.randint(0, 256, (EDGE_H, EDGE_W)) / 256.0
        return (i0, d0, gx0, gy0), i0.copy(), ((0 + half / n) / 4096.0, 0)
    if kind == "one":                                     # |r| = 1: the last bin, not past it
        return (i0, d0, gx0, gy0), np.ones_like(i0), ((4095 + half / n) / 4096.0, 0)
    if kind == "three":                                   # |r| = 3: the last bin too; every row beyond delta
        return (i0, d0, gx0, gy0), np.full_like(i0, 3.0), ((4095 + half / n) / 4096.0, n)
    if kind == "odd":                                     # one depth knocked out: n = 479, half = 240
        i0 = rs.randint(0, 256, (EDGE_H, EDGE_W)) / 256.0
        d0[7, 11] = np.nan
        return (i0, d0, gx0, gy0), i0.copy(), ((0 + 240 / 479) / 4096.0, 0)
    if kind == "half":                                    # the cumulative count meets `half` exactly at the end of bin 3
        i1 = np.full(n, 900.5 / 4096.0)
        i1[rs.permutation(n)[:n // 2]] = 3.5 / 4096.0
        return (i0, d0, gx0, gy0), i1.reshape(EDGE_H, EDGE_W), (4.0 / 4096.0, n // 2)
    if kind == "nan target":                              # more than half the target NaN: delta from bin 4095
        i0 = rs.randint(0, 256, (EDGE_H, EDGE_W)) / 256.0
        i1 = i0.copy()
        i1[:12] = np.nan
        return (i0, d0, gx0, gy0), i1, None
    if kind == "nan depth":                               # no rows at all
        i0 = rs.randint(0, 256, (EDGE_H, EDGE_W)) / 256.0
        return (i0, np.full_like(d0, np.nan), gx0, gy0), i0.copy(), (0.0, 0)
    raise KeyError(kind)


EDGE_KINDS = ("equal", "one", "three", "odd", "half", "nan target", "nan depth")
