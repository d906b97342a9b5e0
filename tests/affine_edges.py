"""Deterministic inputs of tests/test_gpu_affine_edges.py (the affine-illumination kernel's work queue, tap edges, large
angles, mixed batches and skipped levels), with what the checker (tests/affine_ref.py) says about them.
tests/test_affine_edges_cpu.py holds every fixture to the two properties the GPU file relies on -- the checker's
cond(J^T J) leaves affine_ref.pose_bar at the flat 1e-9 x max(1, |x|), and no iteration comes within MARGIN_FLOOR of its
gradient threshold -- so a fixture that drifts fails there, without a device.  Test infrastructure, not collected."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic
from oracle import numpy_twin as twin
from oracle import oracle

import affine_ref as ar
import edge_states

MARGIN_FLOOR = 1e-6                       # test_gpu_affine.MARGIN_FLOOR (the GPU file asserts that the two agree)
GRAD_SCALE = 0.0625                       # image_gradients_scaling_factor of native.make_config


def cfg(mi, mg=None, lo=0.3, hi=5.0):
    """The checker's configuration: affine_ref.optimize hands min_depth / max_depth to system() in every call."""
    nl = len(mi)
    return dict(num_levels=nl, lam=[1.0] * nl, max_iter=list(mi), min_grad=list(mg) if mg else [0.0] * nl,
                min_depth=lo, max_depth=hi)


def twin_pyramid(p, nl):
    """The CPU pyramid of a pair (sizes divisible by 2^(nl-1)): what the CPU pre-checks use in place of the planes the
    GPU tests read back from the device."""
    return twin.build_pyramids(p["gray0"], p["depth0"], p["gray1"], nl, [GRAD_SCALE] * nl)


def flat(ref):
    """Does pose_bar of this checker result equal the flat bar?"""
    return ar.pose_bar(ref["cond"], ref["state"]) <= 1e-9 * max(1.0, float(np.abs(ref["state"]).max()))


# ---- A. the work queue ---------------------------------------------------------------------------------------------
WQ_W, WQ_H, WQ_LEVELS = 24, 20, 2         # level 1: 12x10 = 120 pixels, 2 chunks (waves 2 and 3 idle); level 0: 8 chunks
WQ_MAX_ITER, WQ_MIN_GRAD = [8, 8], [0.5, 0.3]      # A, B, C end after 4-6 / 3-5 iterations, each by its threshold
WQ_SEEDS = (41, 42, 43, 44)               # pairs A, B, C and D (D: all-NaN source depth)
WQ_D = 3
WQ_INITS = 6                              # distinct non-zero initial states of the second list


def work_queue_pairs():
    pairs = [synthetic.make_pair(s, WQ_W, WQ_H, holes=0.02, trans=0.01, rot=0.005) for s in WQ_SEEDS]
    pairs[WQ_D]["depth0"] = np.full_like(pairs[WQ_D]["depth0"], np.nan)
    return pairs


def work_queue_list(n, seed=0):
    """which[k] in 0..3: the pair at position k; D at about one position in ten."""
    rs = np.random.RandomState(seed)
    bad = rs.rand(n) < 0.1
    return np.where(bad, WQ_D, rs.randint(0, WQ_D, n)).astype(int)


def work_queue_inits(n, seed=1):
    """(states[WQ_INITS, 6], pick[n]): position k starts at states[pick[k]]; none is zero."""
    rs = np.random.RandomState(seed)
    states = rs.uniform(-1.0, 1.0, (WQ_INITS, 6)) * np.array([0.008, 0.008, 0.008, 0.004, 0.004, 0.004])
    states[np.abs(states) < 1e-4] = 1e-4
    return states, rs.randint(0, WQ_INITS, n)


# ---- B. exact positions --------------------------------------------------------------------------------------------
SHIFTS = (0.25, -0.25, 0.5, -0.5, 0.75, -0.75)
RANGES = ((0.3, 5.0), (0.5, 2.0))
EXACT_SIZES = {(24, 20): SHIFTS, (75, 53): (0.25, -0.25, 0.5, -0.5)}


def exact_problem(w, h, shift, depth_range):
    """synthetic.half_pixel_problem's planes under the translation (shift, shift, 0) / 64: every projected coordinate is
    exactly c + shift, r + shift.  Depth marks the gate must exclude (both comparisons are strict): a column at min_depth,
    a row at max_depth; under a non-default range also a column at 0.4 and a row at 3.0.  Returns (K, planes, state6)."""
    K, i0, d0, i1, _ = synthetic.half_pixel_problem(w, h)
    lo, hi = depth_range
    d0[:, w // 3] = lo
    d0[h // 3, :] = hi
    if tuple(depth_range) != (0.3, 5.0):
        d0[:, (2 * w) // 3] = 0.4
        d0[(2 * h) // 3, :] = 3.0
    gx, gy = oracle.scharr(i1, GRAD_SCALE)
    return K, (i0, d0, i1, gx, gy), np.array([shift / 64.0, shift / 64.0, 0.0, 0.0, 0.0, 0.0])


def exact_rows(d0, shift):
    """Rows in closed form: depth 1 and the real position strictly inside (-0.5, W - 0.5) x (-0.5, H - 0.5)."""
    h, w = d0.shape
    c, r = np.arange(w) + shift, np.arange(h) + shift
    cin, rin = (c > -0.5) & (c < w - 0.5), (r > -0.5) & (r < h - 0.5)
    return int(np.sum((d0 == 1.0) & rin[:, None] & cin[None, :]))


def exact_bands(shift):
    """The clamp bands rows_loop must report: the outer column and row are kept, taps clamped, only at +-0.25."""
    return {0.25: {"c+", "r+"}, -0.25: {"c-", "r-"}}.get(shift, set())


# ---- C. large angles -----------------------------------------------------------------------------------------------
ANGLE_W, ANGLE_H, ANGLE_SEED = 80, 60, 64   # (seed 61 of test_gpu_large_rotations.py loses every row at roll -0.8 / -1.2)
ANGLE_MAX_ITER = [3, 3]
MOTION_W, MOTION_H = 160, 120
MOTION_MAX_ITER, MOTION_MIN_GRAD = [30], [2.0]


def angle_pair():
    return synthetic.make_pair(ANGLE_SEED, ANGLE_W, ANGLE_H, holes=0.02, trans=0.01, rot=0.004)


def angle_label(state):
    """(axis, sign, branch) of an edge state: branch 2 up to fl(pi/4), 3 beyond (write_pose_constants, gn_device.hpp)."""
    axis = int(np.argmax(np.abs(state[3:])))
    a = state[3 + axis]
    return axis, int(np.sign(a)), 2 if abs(a) <= 0.78539816339744828 else 3


def motion_pairs():
    """[(pair, initial state)] of edge_states.MOTIONS (true yaw 0.5, 0.7, 0.9 rad), started from NEAR."""
    out = []
    for j, m in enumerate(edge_states.MOTIONS):
        p = synthetic.render_pair_with_motion(70 + j, MOTION_W, MOTION_H, m)
        out.append((p, p["motion"] + edge_states.NEAR))
    return out


def nonfinite_batch():
    """Initial states of 10 pairs: 8 healthy small ones with a NaN yaw at position 3 and an inf yaw at position 7."""
    rs = np.random.RandomState(5)
    healthy = rs.uniform(-1.0, 1.0, (8, 6)) * np.array([0.01, 0.01, 0.01, 0.005, 0.005, 0.005])
    bad_nan, bad_inf = np.array(edge_states.BASE), np.array(edge_states.BASE)
    bad_nan[3], bad_inf[3] = np.nan, np.inf
    states = list(healthy)
    states.insert(3, bad_nan)
    states.insert(7, bad_inf)
    return np.array(states), [3, 7]


# ---- D. mixed batch, skipped level -------------------------------------------------------------------------------------
MIX_W, MIX_H, MIX_LEVELS = 80, 60, 3
MIX_MAX_ITER = [4, 4, 4]
MIX_KINDS = ("healthy0", "black", "healthy1", "nan_depth", "seven", "healthy2", "eight", "healthy0", "black", "healthy1",
             "seven", "healthy2")
MIX_SEEDS = dict(healthy0=51, healthy1=52, healthy2=53, black=8, nan_depth=7, seven=54, eight=55)


def sparse_depth(w, h, count, seed):
    """A depth plane of one level: NaN except `count` pixels (depth 1.5 ... 2.5), away from the border."""
    rs = np.random.RandomState(seed)
    d = np.full((h, w), np.nan)
    inner = [(r, c) for r in range(2, h - 2) for c in range(2, w - 2)]
    for i in rs.choice(len(inner), count, replace=False):
        d[inner[i]] = rs.uniform(1.5, 2.5)
    return d


def mixed_pairs():
    """{kind: pair}.  `seven` / `eight`: a black source (the alpha column is exactly zero: an exact zero pivot on both sides,
    as in test_gpu_affine.test_constant_intensity_source, so the flags are defined) whose depth planes, set level by level
    (p["sparse"][level]), hold exactly 7 / 8 valid pixels: one below NP and exactly NP."""
    out = {}
    for kind, seed in MIX_SEEDS.items():
        p = synthetic.make_pair(seed, MIX_W, MIX_H, holes=0.0 if kind in ("black", "nan_depth") else 0.02)
        if kind in ("black", "seven", "eight"):
            p["gray0"] = np.zeros_like(p["gray0"])
        if kind == "nan_depth":
            p["depth0"] = np.full_like(p["depth0"], np.nan)
        if kind in ("seven", "eight"):
            count = 7 if kind == "seven" else 8
            p["sparse"] = [sparse_depth(*twin.level_size(MIX_W, MIX_H, l), count, seed + l) for l in range(MIX_LEVELS)]
        out[kind] = p
    return out


def mixed_pyramid(p):
    pyr = twin_pyramid(p, MIX_LEVELS)
    if "sparse" in p:
        pyr = [(i0, p["sparse"][l], i1, gx, gy) for l, (i0, d0, i1, gx, gy) in enumerate(pyr)]
    return pyr


SKIP_W, SKIP_H = 160, 120
SKIP_MAX_ITER, FULL_MAX_ITER = [5, 0, 5], [5, 5, 5]


def exposure_pair():
    """The 0.8 I + 20 / 255 pair of test_affine_cpu.py and test_gpu_affine.test_gain_and_offset_on_the_device."""
    from test_affine_cpu import exposure_pair as pair
    return pair(31, SKIP_W, SKIP_H)
