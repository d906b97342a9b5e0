"""Deterministic inputs of tests/test_gpu_inverse_system.py (phovo_engine_evaluate_inverse_pairs).  Every
fixture is an image pair (or planes set plane by plane) with the states it is evaluated at; tests/test_inverse_system_cpu.py
holds each of them, on the oracle's CPU planes, to what the GPU file relies on: at least 6 rows and cond(H) <= 1e5 where
the fixture is meant to be well posed (`well_posed`: strips, constant sources and the 5-row systems cannot be), a cost above
1e-12, self-pairs at least SELF_PAIR_KEEP_OUT from the identity (at the identity a self-pair's residual is exactly zero and
the gradient's bar 1e-9 sqrt(H_ii cost) with it: DESIGN.md §15).  Test infrastructure, not collected."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic

import edge_states
import inverse_edges as ie

COND_BAR = 1e5
COST_FLOOR = 1e-12
SELF_PAIR_KEEP_OUT = 0.003

# ---- tile geometries: one level each -----------------------------------------------------------------------------------
# one chunk; a partial chunk; strips; exactly one tile; 1025 pixels (one pixel in the second tile); half a chunk in the second
# tile; 4 tiles; 19 tiles (the finish loop's second and third trip over 8 subsets)
GEOMETRIES = [(8, 8), (7, 5), (45, 1), (1, 45), (32, 32), (41, 25), (33, 32), (75, 53), (160, 120)]
GEOMETRY_SEED = 1


def well_posed_size(w, h):
    """A strip has no gradient across it, and 35 pixels of a smooth render do not span six columns well."""
    return w >= 8 and h >= 8


def geometry_pair(w, h):
    return synthetic.make_pair(GEOMETRY_SEED, w, h, holes=0.02, trans=0.01, rot=0.005)


def three_states(p, seed=0):
    """Zero, the pair's motion, and a random state within 0.02 of the motion."""
    m = np.asarray(p["motion"], dtype=np.float64)
    return np.stack([np.zeros(6), m, m + np.random.RandomState(seed).uniform(-0.02, 0.02, 6)])


# ---- one 640x480 level --------------------------------------------------------------------------------------------------
VGA_SEED = 21


def vga_pair():
    return synthetic.make_pair(VGA_SEED, 640, 480, holes=0.02)


# ---- exact positions, intrinsics, small systems: inverse_edges' parts B, F and G -----------------------------------------
EXACT_CASES = [(w, h, s, r) for (w, h), shifts in ie.EXACT_SIZES.items() for s in shifts for r in ie.RANGES]
K_CASES = [(w, h, s) for (w, h) in ie.K_SIZES for s in ie.K_SHIFTS]
ROWS_CASES = [(layout, count, const) for layout in ie.ROWS_LAYOUTS
              for count, const in ((5, False), (6, False), (7, False), (5, True), (6, True))]
NAN_GX_PIXELS = 200
NAN_SHIFT = np.array([0.1, 0.05, 0.0, 0.0, 0.0, 0.0])     # beside the motion: a band of the target that no row's taps reach


def nan_gx_planes(planes, seed=3):
    """The planes with NaN in NAN_GX_PIXELS pixels of GX0 (drawn among the pixels of valid depth)."""
    i0, d0, gx0, gy0, i1 = planes
    gx = gx0.copy()
    valid = np.flatnonzero((d0.reshape(-1) > 0.3) & (d0.reshape(-1) < 5.0))
    picks = np.random.RandomState(seed).choice(valid, NAN_GX_PIXELS, replace=False)
    gx.reshape(-1)[picks] = np.nan
    return i0, d0, gx, gy0, i1


# ---- levels 1 and 2 of a three-level pool -------------------------------------------------------------------------------
LEVELS_SEED, LEVELS_W, LEVELS_H = 40, 160, 120
LEVELS_MOTION = [0.012, -0.008, 0.01, 0.004, -0.005, 0.006]


def levels_pair():
    return synthetic.render_pair_with_motion(LEVELS_SEED, LEVELS_W, LEVELS_H, LEVELS_MOTION)


# ---- large rotations ----------------------------------------------------------------------------------------------------
def angle_states():
    """0.4 rad of yaw, of pitch and of roll beside a small motion, then every start of edge_states (all finite)."""
    out = []
    for axis in (3, 4, 5):
        s = np.array(edge_states.BASE)
        s[axis] = 0.4
        out.append(s)
    return np.array(out + edge_states.initial_states())


# ---- the aligner's first step ---------------------------------------------------------------------------------------------
STEP_LAMS = (1.0, 0.7)
STEP_START = np.array([0.004, -0.003, 0.005, 0.006, -0.004, 0.003])


def step_pairs():
    """Pairs A, B, C of inverse_edges (24x20) and a 75x53 pair."""
    return ie.work_queue_pairs()[:ie.WQ_D] + [synthetic.make_pair(47, 75, 53, holes=0.02, trans=0.01, rot=0.005)]


# ---- frame pairs of every order -------------------------------------------------------------------------------------------
FOUR_W, FOUR_H, FOUR_SEED = 41, 25, 36
PAIRS_OF_FOUR = [(0, 2), (3, 1), (2, 2), (1, 0), (0, 3)]


def four_frames():
    return synthetic.make_sequence(FOUR_SEED, 4, FOUR_W, FOUR_H, holes=0.02)


def four_states():
    """One state per pair of PAIRS_OF_FOUR, each at least SELF_PAIR_KEEP_OUT from the identity in every entry's sense that
    matters: its norm."""
    rs = np.random.RandomState(5)
    st = rs.uniform(-0.01, 0.01, (len(PAIRS_OF_FOUR), 6))
    st[:, 0] += 0.006
    return st


def pair_of_frames(seq, a, b):
    return dict(gray0=seq["gray"][a], depth0=seq["depth"][a], gray1=seq["gray"][b], depth1=seq["depth"][b], K=seq["K"])


# ---- bit identity ---------------------------------------------------------------------------------------------------------
GROUP_PAIRS = (64 << 20) // (300 * 32 * 8)           # 873 pairs of 300 tiles of 256 B
BOUNDARY_OWN = {0: (1, 2, np.array([-0.015, 0.01, 0.02, -0.008, 0.006, 0.01])),
                872: (2, 0, np.array([0.02, 0.015, -0.01, 0.004, 0.009, -0.007])),
                873: (2, 1, np.array([-0.005, -0.012, 0.018, 0.012, -0.003, 0.005]))}
BOUNDARY_STATE = np.array([0.01, -0.02, 0.015, 0.01, -0.005, 0.008])
