"""Deterministic inputs of tests/test_gpu_geometric_edges.py (the photometric-geometric kernels -- gn_geometric_kernel.hip and
gn_evaluate_geometric_kernels.hip, DESIGN.md §16 and §17 -- at exact tap positions, at large angles, in the work queue with
per-pair start states, in mixed batches, around the rank test, under small-size thresholds and at the evaluate kernel's tile
boundaries), with what the checkers (tests/geometric_ref.py, tests/geometric_system_ref.py) say about them.
tests/test_geometric_edges_cpu.py holds every fixture to what the GPU file relies on -- the three margins of
test_gpu_geometric._compare, cond(H) <= 1e5 where the flat bar is claimed, the closed-form counts, the band and branch
counters -- without a device.  Test infrastructure, not collected."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic
from oracle import oracle

import affine_edges as ae
import edge_states
import geometric_cases as gc
import geometric_ref as gr

MARGIN_FLOOR = 1e-6                       # test_gpu_geometric.MARGIN_FLOOR (the GPU file asserts that the two agree)
START = gc.START


def cfg(mi, mg=None, lam=None, weight=1.0, limit=0.0, lo=0.3, hi=5.0):
    """The checker's configuration: geometric_ref.optimize hands min_depth / max_depth to system() in every call."""
    nl = len(mi)
    as_list = lambda v: [float(v)] * nl if np.isscalar(v) else [float(x) for x in v]
    return dict(num_levels=nl, lam=as_list(1.0 if lam is None else lam), max_iter=list(mi),
                min_grad=as_list(0.0 if mg is None else mg), depth_weight=as_list(weight),
                max_depth_residual=as_list(limit), min_depth=lo, max_depth=hi)


def pyramid(p, nl, mi=None):
    """The CPU pyramid of a pair of any size, pyr[L] = (i0, d0, i1, gx1, gy1, d1), built by the oracle's producers (75x53
    halves to 38x27); the target's depth pyramid is the one a source upload of the target frame leaves.  None on levels
    that mi skips."""
    five = ae.oracle_pyramid(p, nl)
    ocfg = oracle.make_config(num_levels=nl, max_iter=[1] * nl, min_grad=[0.0] * nl)
    _, d1p = oracle.build_source_pyramids(p["gray1"], p["depth1"], ocfg)
    return [five[l] + (d1p[l],) if mi is None or mi[l] > 0 else None for l in range(nl)]


def flat(ref):
    """Does pose_bar of this checker result equal the flat bar?"""
    return gr.pose_bar(ref["cond"], ref["state"]) <= 1e-9 * max(1.0, float(np.abs(ref["state"]).max()))


def margins_hold(ref):
    return ref["margin"] > MARGIN_FLOOR and ref["gate_margin"] > MARGIN_FLOOR and ref["cell_margin"] > gc.CELL_FLOOR


# ---- A. exact positions --------------------------------------------------------------------------------------------
EXACT_SIZES = ae.EXACT_SIZES              # 24x20: shifts +-0.25, +-0.5, +-0.75; 75x53: +-0.25, +-0.5
RANGES = ae.RANGES                        # (0.3, 5.0) and (0.5, 2.0)
EXACT_SIGMA = 2.0
# the residual limit.  Target depths lie on the 1/64 grid and the tap weights on the 1/4 grid, so D1(u, v) - Z' is a
# multiple of 1/1024 (Z' is exactly 1): 0.2003 lies 3.1e-5 from the nearest of them (205 / 1024), a relative margin of 1.6e-4
EXACT_LIMIT = 0.2003


def exact_problem(w, h, shift, depth_range):
    """affine_edges.exact_problem (every projected coordinate exactly c + shift, r + shift; the source depth with a column
    at min_depth and a row at max_depth, and marks at 0.4 / 3.0 under the second range) with a target depth plane on the
    1/64 grid, 1 + randint(-16, 17) / 64, so that the D1 sample and the residual are exact; in it a column at min_depth, a
    row at max_depth, one NaN pixel, and under the second range a column at 0.4 and a row at 3.0 -- which pass the default
    range and fail that one.  Returns (K, planes6, state)."""
    K, (i0, d0, i1, gx, gy), state = ae.exact_problem(w, h, shift, depth_range)
    lo, hi = depth_range
    rs = np.random.RandomState(3)
    d1 = 1.0 + rs.randint(-16, 17, size=(h, w)) / 64.0
    d1[:, w // 2] = lo
    d1[h // 2, :] = hi
    d1[1, 1] = np.nan
    if tuple(depth_range) != (0.3, 5.0):
        d1[:, w // 4] = 0.4
        d1[h // 4, :] = 3.0
    return K, (i0, d0, i1, gx, gy, d1), state


def exact_cfg(depth_range):
    return cfg([1], weight=EXACT_SIGMA, limit=EXACT_LIMIT, lo=depth_range[0], hi=depth_range[1])


# ---- B. large angles -----------------------------------------------------------------------------------------------
# (seed 64, the scene of the affine file, keeps no flat state at roll +0.8 / +1.2 under this objective; of the seeds 61 ...
# 72, 63, 66 and 67 keep one for every axis, sign and branch, and 66 has the smallest largest cond: 3.6e4)
ANGLE_W, ANGLE_H, ANGLE_SEED = 80, 60, 66
ANGLE_MAX_ITER = [3, 3]
ANGLE_SIGMA = 2.0
ANGLE_CLASSES = dict(flat=25, conditioned=0, nonfinite=7)
ANGLE_EVAL_LIMITS = (0.0, 0.0505)         # the evaluate call at the same states: gate off and on
MOTION_W, MOTION_H = ae.MOTION_W, ae.MOTION_H
MOTION_MAX_ITER, MOTION_MIN_GRAD = [30], [3.0]
MOTION_SIGMA, MOTION_LIMIT = 2.0, 0.1


def angle_pair():
    return synthetic.make_pair(ANGLE_SEED, ANGLE_W, ANGLE_H, holes=0.02, trans=0.01, rot=0.004)


def angle_cfg():
    return cfg(ANGLE_MAX_ITER, weight=ANGLE_SIGMA)


def angle_class(ref):
    finite = bool(np.all(np.isfinite(ref["state"])))
    return "flat" if finite and ref["cond"] <= 1e5 else "conditioned" if finite else "nonfinite"


ALL_LABELS = {(axis, sign, branch) for axis in range(3) for sign in (1, -1) for branch in (2, 3)}


def motion_cfg():
    return cfg(MOTION_MAX_ITER, MOTION_MIN_GRAD, weight=MOTION_SIGMA, limit=MOTION_LIMIT)


# ---- C. the work queue with per-pair start states ------------------------------------------------------------------------
WQ_W, WQ_H, WQ_LEVELS = 24, 20, 2
WQ_MAX_ITER, WQ_WEIGHT, WQ_LIMIT = [4, 3], [2.0, 3.0], [0.0505, 0.0]     # test_work_queue_hands_every_pair_its_own_bits
WQ_N = 520
WQ_KINDS = ((0, 1), (0, 2), (3, 1), (4, 5))       # healthy, no depth row, no row, another healthy pair: (source, target) frames


def work_queue_frames():
    """[(gray, depth)] of the six frames of the existing work-queue test."""
    a = synthetic.make_pair(41, WQ_W, WQ_H, holes=0.02, trans=0.01, rot=0.005)
    b = synthetic.make_pair(42, WQ_W, WQ_H, holes=0.02, trans=0.01, rot=0.005)
    return a["K"], [(a["gray0"], a["depth0"]), (a["gray1"], a["depth1"]), (a["gray1"], np.zeros_like(a["depth1"])),
                    (a["gray0"], np.full_like(a["depth0"], np.nan)), (b["gray0"], b["depth0"]), (b["gray1"], b["depth1"])]


def work_queue_pair(frames, kind):
    (g0, d0), (g1, d1) = frames[WQ_KINDS[kind][0]], frames[WQ_KINDS[kind][1]]
    return dict(gray0=g0, depth0=d0, gray1=g1, depth1=d1)


def work_queue_draw():
    """(states[6, 6], pick[WQ_N], which[WQ_N]): position k aligns pair kind which[k] from states[pick[k]]; none is zero."""
    states, pick = ae.work_queue_inits(WQ_N)
    which = np.random.RandomState(4).randint(0, len(WQ_KINDS), WQ_N)
    return states, pick, which


def work_queue_cfg():
    return cfg(WQ_MAX_ITER, weight=WQ_WEIGHT, limit=WQ_LIMIT)


# ---- D. mixed batch, skipped level -------------------------------------------------------------------------------------
MIX_W, MIX_H, MIX_LEVELS = 80, 60, 3
MIX_MAX_ITER, MIX_WEIGHT, MIX_LIMIT = [4, 4, 4], 3.0, 0.1
MIX_KINDS = ("healthy0", "no_target_depth", "healthy1", "nan_source", "target_holes", "healthy2", "healthy0",
             "no_target_depth", "healthy1", "target_holes", "nan_source", "healthy2")
MIX_SEEDS = dict(healthy0=51, healthy1=52, healthy2=53, no_target_depth=14, nan_source=7, target_holes=12)


def mixed_pairs():
    out = {}
    for kind, seed in MIX_SEEDS.items():
        p = gc.holes_pair(seed, MIX_W, MIX_H) if kind == "target_holes" else synthetic.make_pair(seed, MIX_W, MIX_H, holes=0.02)
        if kind == "no_target_depth":
            p["depth1"] = np.zeros_like(p["depth1"])
        if kind == "nan_source":
            p["depth0"] = np.full_like(p["depth0"], np.nan)
        out[kind] = p
    return out


def mixed_cfg():
    return cfg(MIX_MAX_ITER, weight=MIX_WEIGHT, limit=MIX_LIMIT)


SKIP_W, SKIP_H, SKIP_SEED = 160, 120, 31
SKIP_MAX_ITER, FULL_MAX_ITER = [5, 0, 5], [5, 5, 5]
SKIP_WEIGHT, SKIP_LIMIT = 3.0, 0.1


def skip_pair():
    return synthetic.make_pair(SKIP_SEED, SKIP_W, SKIP_H, holes=0.02)


def skip_cfg(mi):
    return cfg(mi, weight=SKIP_WEIGHT, limit=SKIP_LIMIT)


# ---- E. row counts around the rank test ------------------------------------------------------------------------------
ROWS_W, ROWS_H = ae.ROWS_W, ae.ROWS_H     # 24x20: 8 chunks of 64, two per wave
ROWS_LAYOUTS = ae.ROWS_LAYOUTS
ROWS_SEARCH = range(400)                  # tests/test_geometric_edges_cpu.py searches these seeds again
ROWS_SEED = dict(one_chunk=348, four_waves=183)   # the smallest worst cond(H) of the range: 5.3e2, 5.0e2
ROWS_ITER = 3
ROWS_SIGMA = 2.0
ROWS_COUNTS = (5, 6, 7)


def rows_problem(seed, layout, count, target_depth=True):
    """affine_edges.rows_problem (one 24x20 level of random planes, source depth NaN except the first `count` of nine pixels
    at least two from the border, in one chunk or in all four waves) with a target depth plane: random, U(1.5, 2.5) per
    pixel, so its interpolant's derivative varies from row to row as GX1 and GY1 do, and the source depths replaced by the
    target's at the same pixel plus N(0, 0.02), so the depth residuals are centimetres.  Every tap passes the gate; with
    target_depth=False the plane is 0 everywhere and no tap does.  Returns (K, planes6) or None (an unusable seed)."""
    prob = ae.rows_problem(seed, layout, count)
    if prob is None:
        return None
    K, (i0, d0, i1, gx, gy) = prob
    rs = np.random.RandomState(1000 + seed)
    d1 = rs.uniform(1.5, 2.5, d0.shape)
    noise = rs.normal(0.0, 0.02, d0.shape)
    d0 = np.where(np.isfinite(d0), d1 + noise, np.nan)
    return K, (i0, d0, i1, gx, gy, d1 if target_depth else np.zeros_like(d1))


def rows_cfg(mi):
    return cfg(mi, weight=ROWS_SIGMA)


def rows_worst_cond(seed, layout):
    """The largest cond(H) the checker meets on the 6- and the 7-row problem over ROWS_ITER iterations from START (inf:
    unusable -- a repeated pixel, a row or a depth row lost on the way, a non-finite state, a margin missed)."""
    worst = 0.0
    for count in (6, 7):
        prob = rows_problem(seed, layout, count)
        if prob is None:
            return np.inf
        K, planes = prob
        for it in range(1, ROWS_ITER + 1):
            ref = gr.optimize([planes], K, rows_cfg([it]), START)
            if (ref["valid_pixels"] != [count] or ref["depth_rows"] != [count] or ref["flags"]
                    or not np.all(np.isfinite(ref["state"])) or not ref["cell_margin"] > 1e-6):
                return np.inf
        worst = max(worst, ref["cond"])
    return worst


# ---- F. thresholds at small sizes --------------------------------------------------------------------------------------
THR_SIZES = ((24, 20), (75, 53))
THR_SEED = {(24, 20): 41, (75, 53): 45}
THR_MAX_ITER, THR_LAM = [12, 12], [0.7, 0.5]
THR_WEIGHT, THR_LIMIT = [2.0, 3.0], [0.0505, 0.0213]
# each level ends by its threshold: 24x20 after 7 / 5 iterations (levels 0 / 1), 75x53 after 8 / 4; the gradient norms next
# to a threshold stay 11 % of it away or more
THR_MIN_GRAD = {(24, 20): [1.5, 0.4], (75, 53): [25.0, 30.0]}


def threshold_pair(w, h):
    return synthetic.make_pair(THR_SEED[(w, h)], w, h, holes=0.02, trans=0.01, rot=0.005)


def threshold_cfg(w, h):
    return cfg(THR_MAX_ITER, THR_MIN_GRAD[(w, h)], lam=THR_LAM, weight=THR_WEIGHT, limit=THR_LIMIT)


# ---- G. the evaluate kernel's tiles, the aligner's chunk counts --------------------------------------------------------
# 1024 pixels: exactly one tile; 1025: a second tile with one pixel; 8192: 8 tiles, one per subset of the finish kernel; 8256:
# 9 tiles, so subset 0 adds tiles 0 and 8
TILE_SIZES = ((32, 32), (41, 25), (128, 64), (129, 64))
TILE_SEED = 82                            # (of 81 ... 99 the first whose last pixel at 41x25 -- the second tile -- has a depth row at START)
TILE_SIGMA, TILE_LIMITS = 2.0, (0.0, 0.0505)
TILE_ANGLE = np.array(edge_states.BASE)
TILE_ANGLE[3] = 0.8                       # yaw in branch 3: an in-plane turn keeps rows at every size
CHUNK_SIZES = ((8, 24), (32, 24))         # 3 chunks (fewer than waves: wave 0 has 1) and 12 (3 per wave)
CHUNK_MAX_ITER, CHUNK_SIGMA, CHUNK_LIMIT = [5], 2.0, 0.0505


def tile_pair(w, h):
    return synthetic.make_pair(TILE_SEED, w, h, holes=0.02, trans=0.01, rot=0.005)


def tile_states():
    return np.stack([START, TILE_ANGLE])
