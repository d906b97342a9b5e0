"""Deterministic inputs of tests/test_gpu_inverse_edges.py (the inverse-compositional kernel's work queue, exact positions,
the three regimes of its Exp, large angles, step lengths, intrinsics, systems of 5, 6 and 7 rows, a skipped and a long
level), with what the checker (tests/inverse_ref.py) says about them.  tests/test_inverse_edges_cpu.py holds
every fixture to the properties the GPU file relies on -- the checker's cond(J^T J) leaves inverse_ref.pose_bar at the flat
1e-9 x max(1, |x|), no iteration comes within MARGIN_FLOOR of its gradient threshold, the output angles keep clear of the
branch cut of atan2 and of the gimbal lock -- so a fixture that drifts fails there, without a device.  The generic helpers
(the configuration, the CPU pyramids, the work-queue draws, the exact-position planes, the large-angle pairs) are
tests/affine_edges.py's.  Test infrastructure, not collected."""
import contextlib

import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic
from oracle import numpy_twin as twin
from oracle import oracle

import affine_edges as ae
import inverse_ref as ir
from affine_edges import GRAD_SCALE, cfg, work_queue_inits, work_queue_list, work_queue_pairs  # noqa: F401

MARGIN_FLOOR = 1e-6                       # test_gpu_inverse.MARGIN_FLOOR (the GPU file asserts that the two agree)
YAW_ROLL_KEEP_OUT = 1e-3                  # output yaw and roll stay this far from +-pi (the branch cut of atan2)
PITCH_KEEP_OUT = 0.05                     # output pitch stays this far from +-pi/2 (cos(pitch) = 0: yaw and roll undefined)


def source_side(pyr, scharr):
    """A forward aligner's pyramid [(i0, d0, i1, gx1, gy1)] as the checker's [(i0, d0, gx0, gy0, i1)]: the source's gradient
    planes are the Scharr of the source's own intensity level (what a target upload of that frame leaves in the pool)."""
    return [(i0, d0) + tuple(scharr(i0, GRAD_SCALE)) + (i1,) for i0, d0, i1, _, _ in pyr]


def twin_pyramid(p, nl):
    """The CPU pyramid of a pair (sizes divisible by 2^(nl-1)), as test_inverse_cpu.twin_pyramid builds it."""
    return source_side(ae.twin_pyramid(p, nl), twin.scharr)


def oracle_pyramid(p, nl):
    """The CPU pyramid of a pair of any size (75x53 halves to 38x27), built by the oracle's producers."""
    return source_side(ae.oracle_pyramid(p, nl), oracle.scharr)


def flat(ref):
    """Does pose_bar of this checker result equal the flat bar?"""
    return ir.pose_bar(ref["cond"], ref["state"]) <= 1e-9 * max(1.0, float(np.abs(ref["state"]).max()))


def clear_of_the_cuts(state):
    """Output yaw and roll at least YAW_ROLL_KEEP_OUT from +-pi, output pitch at least PITCH_KEEP_OUT from +-pi/2."""
    yaw, pitch, roll = [abs(float(v)) for v in state[3:6]]
    return (np.pi - yaw >= YAW_ROLL_KEEP_OUT and np.pi - roll >= YAW_ROLL_KEEP_OUT
            and abs(0.5 * np.pi - pitch) >= PITCH_KEEP_OUT)


# ---- A. the work queue ---------------------------------------------------------------------------------------------
# pairs, list and initial states: affine_edges' (24x20, two levels, seeds 41 ... 44, D with an all-NaN source depth).  The
# thresholds are this kernel's own: its gradient is in the twist basis and contracted with the source's gradient planes.
WQ_W, WQ_H, WQ_LEVELS, WQ_D, WQ_INITS = ae.WQ_W, ae.WQ_H, ae.WQ_LEVELS, ae.WQ_D, ae.WQ_INITS
WQ_MAX_ITER, WQ_MIN_GRAD = [8, 8], [0.6, 0.5]             # A, B, C end after 4-6 / 3-4 iterations, each by its threshold


# ---- B. exact positions --------------------------------------------------------------------------------------------
SHIFTS, RANGES, EXACT_SIZES = ae.SHIFTS, ae.RANGES, ae.EXACT_SIZES
exact_rows, exact_bands = ae.exact_rows, ae.exact_bands


def exact_problem(w, h, shift, depth_range):
    """affine_edges.exact_problem (every projected coordinate is exactly c + shift, r + shift; marker columns and rows at
    the gate values) with the source's gradient planes: the Scharr of i0.  Returns (K, planes, state6)."""
    K, (i0, d0, i1, _, _), state = ae.exact_problem(w, h, shift, depth_range)
    gx0, gy0 = oracle.scharr(i0, GRAD_SCALE)
    return K, (i0, d0, gx0, gy0, i1), state


def bands_seen(planes, K, state, depth_range):
    """The clamp bands the rows of inverse_ref.rows_loop fall in: 'c-' / 'c+' / 'r-' / 'r+' where a tap column / row is
    clamped at the low / high edge (affine_ref.rows_loop's names), and the number of rows."""
    R, t = ir.eigen_rt(state)
    _, _, rows = ir.rows_loop(planes, 0, K, R, t, *depth_range)
    i0, d0 = planes[0], planes[1]
    h, w = i0.shape
    seen = set()
    for k in np.flatnonzero(rows):
        rr, cc = divmod(int(k), w)
        pz = d0[rr, cc]
        P = R @ np.array([(cc - K[0, 2]) * pz / K[0, 0], (rr - K[1, 2]) * pz / K[1, 1], pz]) + t
        fc, fr = np.floor(P[0] * K[0, 0] / P[2] + K[0, 2]), np.floor(P[1] * K[1, 1] / P[2] + K[1, 2])
        seen |= {name for name, hit in (("c-", fc < 0), ("c+", fc + 1 > w - 1), ("r-", fr < 0), ("r+", fr + 1 > h - 1)) if hit}
    return seen, int(rows.sum())


# ---- C. Exp's three regimes, from one iteration ------------------------------------------------------------------------
# One iteration from the zero state: (R, t) = Exp(xi), xi = -lambda H^-1 g.  lambda is chosen so that |omega| is the target:
# the Taylor side (th^2 < 1e-8), both lanes in the polynomials (th <= pi/4), th beyond pi/4 with th/2 inside, both beyond.
EXP_W, EXP_H = 24, 20
EXP_SEEDS = (41, 42, 43)
EXP_TARGETS = (5e-5, 9.9e-5, 1.01e-4, 0.3, 0.783, 0.80, 1.2, 2.0, 3.0)
QUARTER_PI = 0.78539816339744828           # fl(pi/4): pose_sincos_lane0 takes its polynomials up to here


def exp_pair(seed):
    return synthetic.make_pair(seed, EXP_W, EXP_H, holes=0.02, trans=0.01, rot=0.005)


def exp_lambda(planes, K, target):
    """(lambda, xi): the step length at which the first iteration from the zero state turns by `target` radians."""
    g, Hm, _ = ir.system(planes, 0, K, np.eye(3), np.zeros(3))
    step = np.linalg.solve(Hm, g)
    lam = target / float(np.linalg.norm(step[3:]))
    return lam, -lam * step


def exp_regime(xi):
    """(Taylor side, th > pi/4, th/2 > pi/4) of a twist, with the kernel's own comparisons."""
    th2 = float(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5])
    th = np.sqrt(th2)
    return th2 < ir.TAYLOR_BELOW, bool(th > QUARTER_PI), bool(0.5 * th > QUARTER_PI)


# ---- D. large angles -----------------------------------------------------------------------------------------------
ANGLE_W, ANGLE_H, ANGLE_MAX_ITER = ae.ANGLE_W, ae.ANGLE_H, ae.ANGLE_MAX_ITER
angle_pair, nonfinite_batch, motion_pairs = ae.angle_pair, ae.nonfinite_batch, ae.motion_pairs
ANGLE_FINITE, ANGLE_LOST = 28, 4           # of edge_states.initial_states(): the starts with pitch or roll at +-1.2 lose every row
MOTION_W, MOTION_H = ae.MOTION_W, ae.MOTION_H
MOTION_MAX_ITER, MOTION_MIN_GRAD = [30], [2.0]


# ---- E. step length ------------------------------------------------------------------------------------------------
STEP_LAMS = ae.STEP_LAMS
STEP_FIXED = [4, 4]
STEP_MAX_ITER = [12, 12]                   # under part A's thresholds: every level ends by its threshold with these lambdas
STEP_WIDE_W, STEP_WIDE_H = ae.STEP_WIDE_W, ae.STEP_WIDE_H
STEP_WIDE_MAX_ITER, STEP_WIDE_MIN_GRAD = [12, 16], [1.0, 5.0]       # 4-8 / 8-12 iterations
step_pairs = ae.step_pairs


def step_configs(wide):
    """[(name, max_iter, min_grad)]: fixed iterations, and thresholds."""
    return [("fixed", STEP_FIXED, None),
            ("threshold", STEP_WIDE_MAX_ITER if wide else STEP_MAX_ITER, STEP_WIDE_MIN_GRAD if wide else WQ_MIN_GRAD)]


# ---- F. intrinsics -------------------------------------------------------------------------------------------------
# (every other inverse fixture has fx == fy: the row's J[0] = gx fx / pz and J[1] = gy fy / pz are the kernel's own lines)
K_SIZES, K_SHIFTS, K_MAX_ITER, K_INIT = ae.K_SIZES, ae.K_SHIFTS, ae.K_MAX_ITER, ae.K_INIT
intrinsics_problem = ae.intrinsics_problem
ROW_MUTANTS = ("fx_fx", "fy_fy", "fy_fx")   # the focal lengths a wrong row takes for its columns 0 and 1


@contextlib.contextmanager
def row_focal_mutant(kind):
    """inverse_ref with a row whose two image-gradient columns take the wrong focal lengths (the warp keeps the right
    ones): `fx_fx` fx for both, `fy_fy` fy for both, `fy_fx` the two exchanged.  inverse_ref itself is not edited."""
    orig = ir.rows_vectorised

    def mutant(planes, level, K, R, t, min_depth=0.3, max_depth=5.0):
        res, _, rows = orig(planes, level, K, R, t, min_depth, max_depth)
        i0, d0, gx0, gy0, _ = planes
        h, w = i0.shape
        fx, fy, ox, oy = ir._intrinsics(level, K)
        fa, fb = dict(fx_fx=(fx, fx), fy_fy=(fy, fy), fy_fx=(fy, fx))[kind]
        cc, rr = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        pz = d0.reshape(-1)
        with np.errstate(all="ignore"):
            px, py = (cc.reshape(-1) - ox) * pz / fx, (rr.reshape(-1) - oy) * pz / fy
            a0, a1 = gx0.reshape(-1) * fa / pz, gy0.reshape(-1) * fb / pz
            a2 = -(a0 * px + a1 * py) / pz
            J = np.stack([a0, a1, a2, py * a2 - pz * a1, pz * a0 - px * a2, px * a1 - py * a0], axis=1)
        J[~rows] = 0.0
        return res, J, rows
    ir.rows_vectorised = mutant
    try:
        yield
    finally:
        ir.rows_vectorised = orig


# ---- G. five, six and seven rows -----------------------------------------------------------------------------------
ROWS_W, ROWS_H = 24, 20                   # 480 pixels: 8 chunks of 64 (the last one half full), two per wave
ROWS_LAYOUTS = ("one_chunk", "four_waves")
ROWS_SEARCH = range(300)                  # tests/test_inverse_edges_cpu.py searches these seeds again
ROWS_SEED = dict(one_chunk=138, four_waves=181)
ROWS_ITER = 3
ROWS_DRAWN = 7


def rows_problem(seed, layout, count, constant_source=False):
    """One 24x20 level, set plane by plane: depth NaN except `count` pixels at least two pixels from the border with depths
    from U(0.5, 4.5) -- the first `count` of seven drawn once, so that 5, 6 and 7 share their planes -- I0 from U(0, 1),
    I1 = I0 + N(0, 0.01), GX0 and GY0 from U(-1, 1).  `one_chunk`: all seven in chunk 2 (raster indices 128 ... 191, wave
    2); `four_waves`: pixel j in a chunk of wave j mod 4, so the system is summed from rows of all four waves.
    `constant_source`: I0 = 0.5 and zero gradient planes -- every row, and so H, is exactly zero.
    Returns (K, planes), or None where a pixel was drawn twice."""
    w, h = ROWS_W, ROWS_H
    rs = np.random.RandomState(seed)
    inner = [r * w + c for r in range(2, h - 2) for c in range(2, w - 2)]
    if layout == "one_chunk":
        picks = rs.choice([k for k in inner if k // 64 == 2], ROWS_DRAWN, replace=False)
    else:
        picks = [rs.choice([k for k in inner if (k // 64) % 4 == j % 4]) for j in range(ROWS_DRAWN)]
    if len({int(k) for k in picks}) < ROWS_DRAWN:                # (four_waves draws with replacement: such a seed is unusable)
        return None
    depths = rs.uniform(0.5, 4.5, ROWS_DRAWN)
    i0 = rs.uniform(0.0, 1.0, (h, w))
    i1 = i0 + rs.normal(0.0, 0.01, (h, w))
    gx, gy = rs.uniform(-1.0, 1.0, (h, w)), rs.uniform(-1.0, 1.0, (h, w))
    if constant_source:
        i0, gx, gy = np.full((h, w), 0.5), np.zeros((h, w)), np.zeros((h, w))
    d0 = np.full((h, w), np.nan)
    for k, z in list(zip(picks, depths))[:count]:
        d0[divmod(int(k), w)] = z
    return synthetic.intrinsics(w, h), (i0, d0, gx, gy, i1)


def rows_worst_cond(seed, layout):
    """The largest cond(J^T J) the checker meets on the 6- and the 7-row problem over ROWS_ITER iterations (inf: unusable --
    a repeated pixel, a row lost on the way, a non-finite state)."""
    worst = 0.0
    for count in (6, 7):
        prob = rows_problem(seed, layout, count)
        if prob is None:
            return np.inf
        K, planes = prob
        for it in range(1, ROWS_ITER + 1):
            ref = ir.optimize([planes], K, cfg([it]))
            if ref["valid_pixels"] != [count] or ref["flags"] or not np.all(np.isfinite(ref["state"])):
                return np.inf
        worst = max(worst, ref["cond"])
    return worst


# (name, layout, rows, constant source) of the four systems that stand among healthy pairs in one enqueue
ROWS_MIXED = (("six", "four_waves", 6, False), ("const_five", "four_waves", 5, True), ("seven", "one_chunk", 7, False),
              ("const_six", "four_waves", 6, True))


# ---- H. a skipped level and a long level ---------------------------------------------------------------------------------
SKIP_W, SKIP_H, SKIP_SEED = ae.SKIP_W, ae.SKIP_H, 31
SKIP_MAX_ITER, FULL_MAX_ITER = ae.SKIP_MAX_ITER, ae.FULL_MAX_ITER
LONG_W, LONG_H, LONG_SEED, LONG_ITER = 80, 60, 5, 50      # the benchmark's count on its own coarsest level size
ORTHONORMAL_BELOW = 1e-13                 # |R^T R - I| of the checker's (R, t) after LONG_ITER compositions


def skip_pair():
    return synthetic.make_pair(SKIP_SEED, SKIP_W, SKIP_H, holes=0.02)


def long_pair():
    return synthetic.make_pair(LONG_SEED, LONG_W, LONG_H, holes=0.02)


def final_rotation(pyr, K, config, init_pose=None):
    """(the checker's record, the rotation matrix its last level ended with): inverse_ref.optimize hands every level's
    final (R, t) to state_from_pose; this listens there."""
    orig = ir.state_from_pose
    seen = []

    def listener(R, t):
        seen.append(np.array(R))
        return orig(R, t)
    ir.state_from_pose = listener
    try:
        ref = ir.optimize(pyr, K, config, init_pose)
    finally:
        ir.state_from_pose = orig
    return ref, seen[-1]
