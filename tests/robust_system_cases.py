"""Deterministic inputs of tests/test_gpu_robust_system.py (phovo_engine_evaluate_robust_pairs).  The image
fixtures are tests/inverse_system_cases.py's (tile geometries, the 640x480 level, the first step's pairs, the small systems,
the NaN planes) and tests/inverse_robust_cases.py's occluder; new here are the placed medians across three tiles, the scale
factors, the given deltas and the group boundary of this call's own formula.  tests/test_robust_system_cpu.py holds each of
them, on the oracle's CPU planes, to what the GPU file relies on: rows, conditioning where the fixture is meant to be well
posed, and the two margins on which exact counts rest (1e-7 bins, 1e-10 in |r| - delta).  Test infrastructure, not
collected."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic

import inverse_robust_cases as rc
import inverse_robust_edges as re_
import inverse_robust_ref as rr
import inverse_system_cases as cs

COND_BAR = cs.COND_BAR
SCALES = (rr.DEFAULT_SCALE, 0.5, 1.0)
UNIT_SCALE = re_.UNIT_SCALE                  # 2^40: every weight is 1 (m >= 2^-13 wherever there is a row)
UNIT_DELTA = 2.0 ** 40                      # a given delta beyond every finite intensity difference

GEOMETRIES = cs.GEOMETRIES
geometry_pair, three_states, well_posed_size, vga_pair = cs.geometry_pair, cs.three_states, cs.well_posed_size, cs.vga_pair

# ---- DESIGN.md §22's occluded fixture -------------------------------------------------------------------------------------
OCCLUDED_SEED, OCCLUDED_SHARE = 5, 0.1


def occluded_pair():
    return rc.occluded_pair(OCCLUDED_SEED, OCCLUDED_SHARE)


# ---- placed medians across three tiles --------------------------------------------------------------------------------
# inverse_robust_edges.PLACED with every count times 6 on a 64x48 level (3 tiles of 1024 pixels; the fullest list fills 2880
# of the 3072).  A bin's 6 c rows are dealt 2 c to every tile, at pixels drawn by one seeded permutation per tile: every
# bin's rows, the median's included, arrive from all three tiles, and no tile alone holds the median the pair has.
TILES_W, TILES_H, TILES_FACTOR, TILES_SEED = 64, 48, 6, 13
TILES_K = np.array([[32.0, 0.0, 32.0], [0.0, 32.0, 24.0], [0.0, 0.0, 1.0]])     # zero pose: every pixel on its own, weights 0


def tiles_placement(name):
    return [(k, TILES_FACTOR * c) for k, c in re_.PLACED[name]]


def tiles_planes(name):
    """(i0, d0, gx0, gy0, i1) of a placement on the three-tile level, and per tile the set of bins it holds."""
    n = TILES_W * TILES_H
    rs = np.random.RandomState(TILES_SEED)
    gx0, gy0 = rs.uniform(-0.5, 0.5, (2, TILES_H, TILES_W))
    perms = [1024 * t + rs.permutation(1024) for t in range(3)]
    i1, d0 = np.zeros(n), np.full(n, np.nan)
    at = 0
    per_tile = [set(), set(), set()]
    for k, count in re_.PLACED[name]:
        for t in range(3):
            px = perms[t][at:at + 2 * count]
            assert len(px) == 2 * count
            i1[px] = (k + 0.5) / 4096.0
            d0[px] = 1.0
            per_tile[t].add(k)
        at += 2 * count
    shape = (TILES_H, TILES_W)
    return (np.zeros(shape), d0.reshape(shape), gx0, gy0, i1.reshape(shape)), per_tile


# ---- the aligner's first step ---------------------------------------------------------------------------------------------
STEP_LAMS, STEP_START, step_pairs = cs.STEP_LAMS, cs.STEP_START, cs.step_pairs

# ---- given deltas ---------------------------------------------------------------------------------------------------------
SMALL_DELTA_SHARE = 0.25                    # of the pair's own median: most rows are outliers
BAD_DELTAS = (np.nan, np.inf, -np.inf, 0.0, -0.0, -1e-3)

# ---- small systems and NaN planes: inverse_system_cases' ---------------------------------------------------------------
ROWS_CASES, NAN_SHIFT, nan_gx_planes = cs.ROWS_CASES, cs.NAN_SHIFT, cs.nan_gx_planes
NAN_I1_PIXELS = 5


def nan_i1_planes(planes, hit, seed=4):
    """The planes with NaN in NAN_I1_PIXELS pixels of I1 among those that rows sample (`hit`:
    inverse_system_ref.sampled_target_pixels)."""
    i1 = planes[4].copy()
    picks = np.random.RandomState(seed).choice(np.flatnonzero(hit.reshape(-1)), NAN_I1_PIXELS, replace=False)
    i1.reshape(-1)[picks] = np.nan
    return planes[:4] + (i1,)


# ---- bit identity -----------------------------------------------------------------------------------------------------------
# the host's formula at 8x8: one tile of 256 B, 16 KiB of histogram and 16 B of (m, delta) per pair within 64 MiB
GROUP_BYTES_PER_PAIR_8X8 = 256 + 16384 + 16
GROUP_PAIRS_8X8 = (64 << 20) // GROUP_BYTES_PER_PAIR_8X8
BOUNDARY_FRAMES, BOUNDARY_SEED = 4, 9
BOUNDARY_STATE = np.array([0.004, -0.006, 0.005, 0.004, -0.003, 0.002])
BOUNDARY_OWN = {0: (1, 2, np.array([-0.005, 0.004, 0.006, -0.003, 0.002, 0.004])),
                GROUP_PAIRS_8X8 - 1: (2, 3, np.array([0.006, 0.005, -0.004, 0.002, 0.003, -0.002])),
                GROUP_PAIRS_8X8: (3, 1, np.array([-0.002, -0.004, 0.006, 0.004, -0.001, 0.002]))}


def boundary_frames():
    return synthetic.make_sequence(BOUNDARY_SEED, BOUNDARY_FRAMES, 8, 8, holes=0.0)


def pair_of_frames(seq, a, b):
    return cs.pair_of_frames(seq, a, b)
