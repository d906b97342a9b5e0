"""Randomised device-vs-checker sweep of the bi-objective (`bi`, gn_biobjective_kernel.hip), trust-region (`tr`,
gn_trust_region_kernel.hip), evaluate (`eval`, gn_evaluate_kernels.hip), affine-illumination (`affine`,
gn_affine_kernel.hip) and sampled-system (`sampled`, gn_evaluate_sampled_kernels.hip) kernels, in the style of
fuzz_parity.py.

    python tests/tools/fuzz_objectives.py [cases=100] [seed=0] [mode=bi|tr|eval|affine|sampled] [big] [angles]

Every case draws (draw_case, pure numpy, so that replay and coverage are testable without a GPU): an odd size with 1-3
levels up to 330x250 (`big`: 340x260 ... 700x500 with 1-2 levels) or a strip 1-5 pixels wide; intrinsics perturbed off
the half-integer grid; depth holes and, with some probability, NaN, negative, +inf, beyond-max source depth and depth
exactly at the bounds of the gate; for `bi` zero, negative, beyond-max (rarely NaN) target depth; a depth range, sometimes
changed between upload and alignment; lambda 1 or 0.7 (`bi`); fixed iteration counts or gradient thresholds; for `tr` the
options of a shipped Ceres file (tests/golden/ceres) or fixed mode; initial states (tests/edge_states.py, and in `angles`
mode fuzz_draws.draw_angle's branches under in-plane motions up to 0.9 rad); for `eval` states around the motion on every
level, fp64 / fp32 / fp16 plane storage and Huber weights on or off; 1, 3 or 40 pairs per launch, whose replicas must be
bit-identical.

Checks: `bi` against biobjective_ref.optimize under test_gpu_objective_edges.BiExpect (iterations, valid pixels, flags,
pose within 1e-9 x max(1, cond / 1e5), capped at 1e-5); `tr` against trust_region_ref under
test_gpu_trust_region.compare_pair (steps, accepted steps, terminations, rows, costs to 1e-9, noise floor); `eval` against
the oracle on the planes as the device stores them under test_gpu_pair_system._check_against.  Knife-edge cases are
counted and printed, not failed: for `bi` and `eval` a case that misses its bar while one ulp of fx moves the checker by
more than a quarter of the bar, for `tr` a case with a decision margin of at most 1e-6 (not compared).  A `tr` case that
misses _check's flat bars is compared again under bars conditioned on the checker's cond(J^T J) (conditioned_allowance:
the pose bar as `bi`'s, and what it carries into costs, Jacobi scaling and gradient norm), with every decision, row count
and flag still exact; the summary counts those cases.  The `eval` tile classes are predicted from the level sizes (the
evaluate path keeps no launch record).

`affine` takes `bi`'s draws (lambda 1 or 0.7 per level included; no target-depth defects) and adds its own after them
(_draw_affine), so that the other modes' draws stay what they were: sizes that do not halve exactly, a quarter of the cases
small enough to aim level 0 at one trip-count class of the kernel's pixel loop (CHUNK_CLASSES) with a full or a partial last
chunk, an exposure change of the target (gain and offset before the u8 clip), gradient thresholds of this objective's
scale.  Device side: objective 3 with the case's lambda and perturbed K, upload under one depth range and alignment under
another, the planes of every level that runs read back, every launch of kind `affine`.  Checker side (_check_affine):
affine_ref.optimize on those planes; every replica has replica 0's bits (state, (alpha, beta), report); iterations, valid
pixels and flags equal; where the checker's state is not finite the device's is not finite in the same entries; otherwise
all 8 entries within affine_ref.pose_bar (1e-9 x max(1, cond / 1e5), capped at 1e-5, x max(1, |x|)) and the gradient norm
within 1e-9 x max(1, |g|), plus |H|_2 sqrt(8) x bar where the bar is scaled.  A case within MARGIN_FLOOR of a gradient
threshold is not compared.  A case that misses is set aside, printed and counted, only if the checker itself is unstable
there -- with fx one ulp larger its counts, flags or finiteness change, or its state moves by more than a quarter of the
bar -- or if it met a system of 1 to 7 rows: the step of such a system is rounding noise on both sides and no report after
it is defined, so RANK_DEFICIENT and the levels that ran before it are compared, nothing after.  The
summary adds, from the checker's results, the cases that passed only under the scaled bar, those that ended non-finite,
the levels under a threshold that ended by it and by their count, and the chunk classes run.

`sampled` takes `eval`'s draws (sizes, strips, perturbed K, source-depth defects, both ranges, storage, Huber deltas per
level, the spread and the edge state of the evaluated states, the batch size) and adds its own after them (_draw_sampled):
the row kind -- slip, corrected or affine, the last on fp64 planes without weights as the engine requires --, (alpha,
beta), 2-4 frames rendered as one sequence with every frame's depth carrying the defects, a (src, tgt) per state from all
ordered pairs of frames (tgt < src and src == tgt included; a frame onto itself is evaluated at least 0.003 from the
identity, where its residual would be rounding noise), small sizes of any parity, and in a tenth of the cases depth that
is valid in 1-12 pixels only.  Device side: every level at up to 3 (src, tgt, state); further pairs are replicas, which
must carry their original's bytes; the planes of every level and frame read back.  Checker side (_check_sampled):
sampled_system_ref.system6 / system8 under sampled_system_ref.check_against; no rows: the all-zero record with
RANK_DEFICIENT; fewer rows than columns: the flag and the values.  A miss is set aside, printed and counted, only under
`eval`'s rule -- one ulp of fx moves the checker's own answer by more than a quarter of the bar or changes its row count.
The summary adds the systems checked, the empty ones and those of fewer rows than columns, and the coverage classes
(SAMPLED_CLASSES) of the draws.

One line per failure, a summary, exit status 1 on any failure.  FUZZ_ONLY=12,345 runs only those cases, with the draws of
the full sweep.  The checkers run in FUZZ_JOBS worker processes (default: up to 12), which never touch the GPU.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
from fuzz_draws import draw_angle  # noqa: E402

MODES = ("bi", "tr", "eval", "affine", "sampled")
CERES_FILES = ("config_3_level_optimization_ceres.yml", "config_4_level_optimization_ceres.yml",
               "config_5_level_optimization_ceres.yml", "config_only_level_0_ceres.yml",
               "config_only_level_1_ceres.yml", "config_only_level_2_ceres.yml")
SRC_DEFECTS = ("nan", "negative", "inf", "beyond_max", "at_min", "at_max")
TGT_DEFECTS = ("zero", "negative", "beyond_max", "nan")
# LDS budget of one workgroup (gn_device.hpp LDS_LIMIT) and a bound of the fixed part: the host-side guess of the geometry
# the planners (gn_plan_level_biobjective / _trust_region) choose, for the coverage test; the sweep records the real one
LDS_LIMIT, LDS_FIXED = 160 * 1024, 4096
STATES = None
# gn_affine_kernel.hip has one geometry; what differs from level to level is the trip count of its pixel loop, a two-chunk
# software pipeline over four waves: n_chunks = ceil(n / 64) of 1 (three idle waves), 2-3 (idle waves), 4 (one chunk per
# wave), 5-7 (one or two chunks per wave), 8 (two per wave), 9-12 (the loop's second trip on some waves), 13 and more
CHUNK_CLASSES = ("chunks1", "chunks2-3", "chunks4", "chunks5-7", "chunks8", "chunks9-12", "chunks13+")
MARGIN_FLOOR = 1e-6                       # test_gpu_affine.MARGIN_FLOOR
# the `affine` sweeps of tests/test_gpu_affine_sweep.py: (flags, cases, seed); tests/test_affine_sweep_cpu.py holds their
# draws to full coverage, and the checker on the first one's to the caps, without a device
AFFINE_SWEEPS = (((), 300, 14), (("angles",), 150, 41), (("big",), 40, 52))
# the `sampled` sweeps of tests/test_gpu_sampled_sweep.py, held to full coverage by tests/test_sampled_sweep_cpu.py
SAMPLED_SWEEPS = (((), 300, 14), (("angles",), 150, 41), (("big",), 40, 52))
SAMPLED_KINDS = ("slip", "corrected", "affine")         # the row kinds of gn_evaluate_sampled_kernels.hip
PAIR_RANK_DEFICIENT, PAIR_NONFINITE = 4, 1              # phovo_hip.h (tests/test_sampled_sweep_cpu.py holds them to native)


def _edge_states():
    global STATES
    if STATES is None:
        import edge_states
        STATES = edge_states.initial_states()
    return STATES


def level_size(w, h, level):
    for _ in range(level):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def device_level_size(w, h, level):
    """The size the engine gives a level of any image (engine.cpp level_dims: cvRound(w / 2^level), halves to even)."""
    return int(np.rint(w / 2.0 ** level)), int(np.rint(h / 2.0 ** level))


def predicted_geometry(mode, n):
    if mode == "eval":
        tiles = -(-(-(-n // 64)) // 16)
        return "tiles1" if tiles == 1 else "tiles2-16" if tiles <= 16 else "tiles17+"
    own = 4 * n + 8 * -(-n // 64)
    return "lds256" if LDS_FIXED + own <= LDS_LIMIT // 2 else "lds512" if LDS_FIXED + own <= LDS_LIMIT else "hbm512"


def chunk_class(n):
    nc = -(-n // 64)
    return CHUNK_CLASSES[0 if nc == 1 else 1 if nc <= 3 else 2 if nc == 4 else 3 if nc <= 7 else 4 if nc == 8 else
                         5 if nc <= 12 else 6]


def _draw_affine(rs, c):
    """The draws of `affine` alone, after all others (the other modes' streams do not see them): arbitrary sizes (the
    planes are read back from the device, so a level need not halve exactly), a quarter of the cases small enough to aim
    at one chunk class of the pixel loop, an exposure change of the target, thresholds of this objective's scale."""
    unit = 2 ** (c["nl"] - 1)
    odd = [int(rs.randint(0, unit)), int(rs.randint(0, unit))]
    small = rs.rand() < 0.25
    nc = [1, int(rs.randint(2, 4)), 4, int(rs.randint(5, 8)), 8, int(rs.randint(9, 13)), int(rs.randint(13, 30))][
        int(rs.randint(0, len(CHUNK_CLASSES)))]
    full = rs.rand() < 0.3
    n = 64 * (nc - 1) + int(rs.randint(17, 64))
    sh, fh = int(rs.randint(3, 17)), int(rs.choice([4, 8, 16]))
    if c["size_class"] != "strip":
        if small:                                   # level 0 has nc chunks, the last one full or partial
            # (at least 3 wide: the coarsest of three levels then still has a pixel, device_level_size)
            c.update(size_class="small", w=64 * nc // fh if full else max(n // sh, 3), h=fh if full else sh)
        else:
            c.update(w=c["w"] + odd[0], h=c["h"] + odd[1])
    gain, offset = float(rs.uniform(-0.25, 0.2)), float(rs.uniform(-0.06, 0.1))
    c["exposure"] = [gain, offset] if rs.rand() < 0.7 else None
    # thresholds 0.05 ... 90 in place of 1 ... 300: with at most 6 iterations per level from these starts, ||g|| (a sum
    # over the level's rows) passes 0.3 ... 2.0, where DESIGN.md §14's converged fixtures end, on few levels only
    scale = float(rs.choice([0.05, 0.1, 0.3]))
    c["min_grad"] = [m * scale for m in c["min_grad"]]


def _draw_sampled(rs, c):
    """The draws of `sampled` alone, after all others: the row kind (affine: fp64 planes and no Huber weights, as the
    engine requires), the (alpha, beta) of the eight-column states, 2-4 frames rendered as one sequence, a (src, tgt) per
    state from ALL ordered pairs (tgt < src and src == tgt included), some small sizes of any parity (1 to 11 tiles) and,
    in a tenth of the cases, source depth that is valid in 1-12 pixels of a frame only: systems of fewer rows than
    columns."""
    kind = SAMPLED_KINDS[int(rs.randint(0, 3))]
    alpha, beta = float(rs.uniform(-0.25, 0.2)), float(rs.uniform(-0.06, 0.1))
    nf = int(rs.randint(2, 5))
    pairs = [[int(rs.randint(0, nf)), int(rs.randint(0, nf))] for _ in range(3)]
    small = rs.rand() < 0.15
    sw, sh = int(rs.randint(8, 121)), int(rs.randint(6, 91))
    sparse, is_sparse = int(rs.randint(1, 13)), rs.rand() < 0.1
    c.update(kind=kind, illum=[alpha, beta], n_frames=nf, pairs=pairs, sparse=sparse if is_sparse else None)
    if kind == "affine":
        c.update(storage=0, huber=None)
    if small and c["size_class"] != "strip":
        c.update(size_class="small", w=sw, h=sh)


def draw_case(rs, mode, flags):
    """All random draws of one case, in a fixed order whatever is drawn: a dict of plain values (the images are rendered
    from `seed` and the per-pixel defects from `defect_seed` when the case runs)."""
    big, angles = "big" in flags, "angles" in flags
    c = dict(mode=mode)
    kind = rs.rand()
    nl = int(rs.randint(1, 3 if big else 4))
    unit = 2 ** (nl - 1)
    w = int(rs.randint(340, 701) if big else rs.randint(16, 331)) // unit * unit + (unit if rs.rand() < 0.5 else 0)
    h = int(rs.randint(260, 501) if big else rs.randint(12, 251)) // unit * unit + (unit if rs.rand() < 0.5 else 0)
    w, h = max(w, 8 * unit), max(h, 8 * unit)
    strip_w, strip_h = int(rs.randint(1, 6)), int(rs.randint(12, 121))
    if kind < 0.12:
        c.update(size_class="strip", nl=1, w=strip_w, h=strip_h)
    else:
        c.update(size_class="big" if big else "normal", nl=nl, w=w, h=h)
    nl = c["nl"]
    c["seed"] = int(rs.randint(0, 2 ** 31 - 1))
    c["defect_seed"] = int(rs.randint(0, 2 ** 31 - 1))
    c["holes"] = float(rs.choice([0.0, 0.02, 0.2]))
    c["trans"] = float(rs.choice([0.002, 0.02, 0.08]))
    c["rot"] = float(rs.choice([0.001, 0.01, 0.05]))
    motion = np.concatenate([rs.uniform(-1, 1, 3) * c["trans"], [rs.uniform(-0.9, 0.9)], rs.uniform(-0.01, 0.01, 2)])
    c["motion"] = motion.tolist() if angles else None
    perturb = rs.rand() < 0.6
    kp = [float(rs.uniform(-3, 3)), float(rs.uniform(-3, 3)), float(rs.uniform(0.9, 1.1)), float(rs.uniform(0.9, 1.1))]
    c["k_perturb"] = kp if perturb else None
    with_src = rs.rand() < 0.6
    src = [d for d in SRC_DEFECTS if rs.rand() < 0.5]
    c["src_defects"] = src if with_src else []
    tgt = [d for d in TGT_DEFECTS if rs.rand() < (0.05 if d == "nan" else 0.5)]
    with_tgt = rs.rand() < 0.6
    c["tgt_defects"] = tgt if (with_tgt and mode == "bi") else []
    rk = int(rs.randint(0, 4))
    lo_hi = [float(rs.uniform(0.2, 0.9)), float(rs.uniform(2.5, 6.0))]
    c["range"] = [0.3, 5.0] if rk < 2 else [0.5, 3.0] if rk == 2 else lo_hi
    uk = rs.rand()
    up = [float(rs.uniform(0.2, 0.9)), float(rs.uniform(2.5, 6.0))]
    c["upload_range"] = up if uk < 0.35 else list(c["range"])
    fixed = rs.rand() < 0.5
    max_iter = [int(rs.randint(0, 7)) for _ in range(nl)]
    if sum(max_iter) == 0:
        max_iter[-1] = 3
    mg = [float(rs.choice([1.0, 30.0, 300.0])) for _ in range(nl)]
    c["max_iter"] = max_iter
    c["min_grad"] = [0.0] * nl if fixed else mg
    lam = [float(rs.choice([1.0, 0.7])) for _ in range(nl)]
    c["lam"] = lam if mode in ("bi", "affine") else [1.0] * nl
    ceres = int(rs.randint(0, len(CERES_FILES) + 2))
    c["ceres"] = CERES_FILES[ceres] if ceres < len(CERES_FILES) else "fixed"
    c["tr_max_iter"] = [int(rs.randint(0, 7)) for _ in range(nl)]
    if sum(c["tr_max_iter"]) == 0:
        c["tr_max_iter"][-1] = 4
    ik = rs.rand()
    small = (rs.uniform(-1, 1, 6) * np.array([0.02, 0.02, 0.02, 0.01, 0.01, 0.01])).tolist()
    edge = int(rs.randint(0, 32))
    ang = [draw_angle(rs, axis, motion[3 + axis]) for axis in range(3)] if angles else None
    if angles:
        c["init"] = small[:3] + ang
    else:
        c["init"] = None if ik < 0.3 else small if ik < 0.75 else ("edge", edge)
    c["storage"] = int(rs.randint(0, 3)) if mode in ("eval", "sampled") else 0
    c["huber"] = [float(rs.choice([0.02, 0.05, 0.1])) for _ in range(nl)] if rs.rand() < 0.5 else None
    if mode not in ("eval", "sampled"):
        c["huber"] = None
    c["eval_spread"] = float(rs.choice([0.0, 0.003, 0.02]))
    c["eval_edge"] = int(rs.randint(0, 32)) if rs.rand() < 0.25 else None
    c["n_pairs"] = int(rs.choice([1, 3, 40]))
    if mode == "affine":
        _draw_affine(rs, c)
    if mode == "sampled":
        _draw_sampled(rs, c)
    return c


def draw_cases(cases, seed, mode, flags, only=None):
    """{case: draw} of the first `cases` cases of a sweep (those in `only`, when given): every case is drawn either way,
    so that a replay draws exactly what the full sweep draws."""
    rs = np.random.RandomState(seed)
    out = {}
    for case in range(cases):
        d = draw_case(rs, mode, flags)
        if only is None or case in only:
            out[case] = d
    return out


def case_key(d):
    return repr(sorted(d.items()))


def level_geometries(d):
    if d["mode"] == "sampled":
        return {predicted_geometry("eval", int(np.prod(device_level_size(d["w"], d["h"], l)))) for l in range(d["nl"])}
    levels = [l for l in range(d["nl"]) if d["mode"] == "eval" or
              (d["tr_max_iter"] if d["mode"] == "tr" else d["max_iter"])[l] > 0]
    if d["mode"] == "affine":
        sizes = [int(np.prod(device_level_size(d["w"], d["h"], l))) for l in levels]
        return {chunk_class(n) for n in sizes} | {"last_partial" if n % 64 else "last_full" for n in sizes}
    return {predicted_geometry(d["mode"], int(np.prod(level_size(d["w"], d["h"], l)))) for l in levels}


def coverage(draws, mode):
    """How often the draws reach each size class, geometry, depth defect and range change (for the coverage test)."""
    cov = {f"size_{k}": 0 for k in ("normal", "strip", "big")}
    cov.pop("size_big")
    if mode == "sampled":
        return coverage_sampled(draws)
    geos = ["tiles1", "tiles2-16", "tiles17+"] if mode == "eval" else ["lds256", "lds512", "hbm512"]
    if mode == "affine":
        geos = list(CHUNK_CLASSES) + ["last_partial", "last_full"]
        cov.update(size_small=0, k_perturb=0, exposure=0, no_exposure=0)
    cov.update({g: 0 for g in geos})
    cov.update({f"src_{k}": 0 for k in SRC_DEFECTS})
    if mode == "bi":
        cov.update({f"tgt_{k}": 0 for k in TGT_DEFECTS})
    if mode in ("bi", "affine"):
        cov["lambda_0.7"] = 0
    if mode == "eval":
        cov.update({f"storage_{k}": 0 for k in range(3)})
        cov["huber"] = 0
    if mode == "tr":
        cov.update({"ceres_file": 0, "ceres_fixed": 0})
    cov.update(range_changed=0, range_non_default=0, pairs_1=0, pairs_3=0, pairs_40=0, init_edge=0)
    for d in draws:
        cov[f"size_{d['size_class']}"] = cov.get(f"size_{d['size_class']}", 0) + 1
        for g in level_geometries(d):
            cov[g] += 1
        for k in d["src_defects"]:
            cov[f"src_{k}"] += 1
        for k in d["tgt_defects"]:
            cov[f"tgt_{k}"] += 1
        if mode in ("bi", "affine"):
            cov["lambda_0.7"] += int(0.7 in d["lam"])
        if mode == "affine":
            cov["k_perturb"] += int(d["k_perturb"] is not None)
            cov["exposure" if d["exposure"] is not None else "no_exposure"] += 1
        if mode == "eval":
            cov[f"storage_{d['storage']}"] += 1
            cov["huber"] += int(d["huber"] is not None)
        if mode == "tr":
            cov["ceres_fixed" if d["ceres"] == "fixed" else "ceres_file"] += 1
        cov["range_changed"] += int(d["upload_range"] != d["range"])
        cov["range_non_default"] += int(d["range"] != [0.3, 5.0])
        cov[f"pairs_{d['n_pairs']}"] += 1
        cov["init_edge"] += int(isinstance(d["init"], tuple) or (mode != "affine" and d["eval_edge"] is not None))
    return cov


SAMPLED_CLASSES = (tuple(f"kind_{k}" for k in SAMPLED_KINDS) + tuple(f"storage_{k}" for k in range(3)) +
                   ("huber", "no_huber", "tiles1", "tiles2-16", "tiles17+", "k_perturb", "range_changed", "level1+",
                    "size_strip", "tgt_not_src+1", "tgt_before_src", "src_is_tgt", "pairs_1", "pairs_3", "pairs_40"))


def sampled_pairs_run(d):
    """The (src, tgt) of the states a `sampled` case evaluates: the first min(3, n_pairs) of its drawn pairs."""
    return d["pairs"][:min(3, d["n_pairs"])]


def coverage_sampled(draws):
    """How often the draws of `sampled` reach each class of SAMPLED_CLASSES (storage and Huber under the six-column kinds,
    the frame-pair classes over the pairs that run)."""
    cov = {k: 0 for k in SAMPLED_CLASSES}
    for d in draws:
        cov[f"kind_{d['kind']}"] += 1
        if d["kind"] != "affine":
            cov[f"storage_{d['storage']}"] += 1
            cov["huber" if d["huber"] is not None else "no_huber"] += 1
        for g in level_geometries(d):
            cov[g] += 1
        cov["k_perturb"] += int(d["k_perturb"] is not None)
        cov["range_changed"] += int(d["upload_range"] != d["range"])
        cov["level1+"] += int(d["nl"] > 1)
        cov["size_strip"] += int(d["size_class"] == "strip")
        run = sampled_pairs_run(d)
        cov["tgt_not_src+1"] += int(any(t != s + 1 for s, t in run))
        cov["tgt_before_src"] += int(any(t < s for s, t in run))
        cov["src_is_tgt"] += int(any(t == s for s, t in run))
        cov[f"pairs_{d['n_pairs']}"] += 1
        if d["size_class"] == "big":                # (as coverage(): the class exists only where a draw has it)
            cov["size_big"] = cov.get("size_big", 0) + 1
    return cov


# ---- running a case ------------------------------------------------------------------------------------------------
def render(d):
    """The pair of a case: images, perturbed K, source and target depth with their defects, the initial state."""
    from phovo_amd import synthetic
    w, h = d["w"], d["h"]
    rw = max(w, 64) if w < 8 else w
    if d["motion"] is not None:
        p = synthetic.render_pair_with_motion(d["seed"], rw, h, np.array(d["motion"]), d["holes"])
    else:
        p = synthetic.make_pair(d["seed"], rw, h, holes=d["holes"], trans=d["trans"], rot=d["rot"])
    p = dict(p)
    K = p["K"].copy()
    if w < 8:                                       # a strip of a 64-pixel-wide render, principal point moved with the crop
        for k in ("gray0", "depth0", "gray1", "depth1"):
            p[k] = np.ascontiguousarray(p[k][:, 30:30 + w])
        K[0, 2] -= 30.0
    if d["k_perturb"] is not None:
        K[0, 2] += d["k_perturb"][0]
        K[1, 2] += d["k_perturb"][1]
        K[0, 0] *= d["k_perturb"][2]
        K[1, 1] *= d["k_perturb"][3]
    p["K"] = K
    lo, hi = d["range"]
    rs = np.random.RandomState(d["defect_seed"])
    d0 = np.array(p["depth0"], dtype=np.float64)
    for k, v in (("nan", np.nan), ("negative", -1.0), ("inf", np.inf), ("beyond_max", hi + 2.5), ("at_min", lo),
                 ("at_max", hi)):
        m = rs.rand(h, w) < 0.01
        if k in d["src_defects"]:
            d0[m] = v
    d1 = np.array(p["depth1"], dtype=np.float64)
    for k, v in (("zero", 0.0), ("negative", -0.7), ("beyond_max", hi + 4.0), ("nan", np.nan)):
        m = rs.rand(h, w) < 0.01
        if k in d["tgt_defects"]:
            d1[m] = v
    p["depth0"], p["depth1"] = d0, d1
    if d.get("exposure") is not None:               # (affine) the target under another exposure, clipped like a camera's
        gain, offset = d["exposure"]
        g1 = (1.0 + gain) * p["gray1"].astype(np.float64) + 255.0 * offset
        p["gray1"] = np.clip(np.rint(g1), 0, 255).astype(np.uint8)
    init = d["init"]
    if isinstance(init, tuple):
        init = _edge_states()[init[1]]
    p["init"] = None if init is None else np.array(init, dtype=np.float64)
    return p


def state_of_pose(T):
    """(x, y, z, yaw, pitch, roll) of a 4x4 pose with R = Rz(yaw) Ry(pitch) Rx(roll), |pitch| < pi / 2 (se3.eigen_pose)."""
    R = T[:3, :3]
    return np.array([T[0, 3], T[1, 3], T[2, 3], np.arctan2(R[1, 0], R[0, 0]), np.arcsin(np.clip(-R[2, 0], -1.0, 1.0)),
                     np.arctan2(R[2, 1], R[2, 2])])


def render_sequence(d):
    """The frames of a `sampled` case: n_frames views of one plane scene under chained motions of the case's size (in
    `angles` mode the first step is the case's motion), the perturbed K, every frame's depth with the case's defects (and,
    for `sparse`, valid in that many pixels only), the true relative state of every ordered pair, the states to evaluate."""
    from phovo_amd import se3, synthetic
    w, h, nf = d["w"], d["h"], d["n_frames"]
    rw = max(w, 64) if w < 8 else w
    rs = np.random.RandomState(d["seed"])
    scene = synthetic.Scene(d["seed"])
    K0 = synthetic.intrinsics(rw, h)
    poses, T = [], np.eye(4)
    for f in range(nf):
        if f > 0:
            m = synthetic.random_motion(rs, d["trans"], d["rot"])
            T = se3.eigen_pose(d["motion"] if (f == 1 and d["motion"] is not None) else m) @ T
        poses.append(T.copy())
    frames = [synthetic.render(scene, poses[f], rw, h, K0, d["holes"], hole_seed=d["seed"] % 10007 * 100003 + f)
              for f in range(nf)]
    gray = [g for g, _ in frames]
    depth = [np.array(z, dtype=np.float64) for _, z in frames]
    K = K0.copy()
    if w < 8:
        gray = [np.ascontiguousarray(g[:, 30:30 + w]) for g in gray]
        depth = [np.ascontiguousarray(z[:, 30:30 + w]) for z in depth]
        K[0, 2] -= 30.0
    if d["k_perturb"] is not None:
        K[0, 2] += d["k_perturb"][0]
        K[1, 2] += d["k_perturb"][1]
        K[0, 0] *= d["k_perturb"][2]
        K[1, 1] *= d["k_perturb"][3]
    lo, hi = d["range"]
    rs = np.random.RandomState(d["defect_seed"])
    for z in depth:
        for k, v in (("nan", np.nan), ("negative", -1.0), ("inf", np.inf), ("beyond_max", hi + 2.5), ("at_min", lo),
                     ("at_max", hi)):
            m = rs.rand(h, w) < 0.01
            if k in d["src_defects"]:
                z[m] = v
        keep = rs.permutation(h * w)[:d["sparse"] or 0]
        if d["sparse"] is not None:
            flat = np.full(h * w, np.nan)
            flat[keep] = z.reshape(-1)[keep]
            z[...] = flat.reshape(h, w)
    run = sampled_pairs_run(d)
    rs = np.random.RandomState(d["defect_seed"] + 1)
    states = []
    for s, t in run:
        base = np.zeros(6) if s == t else state_of_pose(poses[t] @ np.linalg.inv(poses[s]))
        # a frame warped onto itself by the identity has a residual of rounding noise only (cost about 1e-28), under which
        # the relative bars on gradient and cost say nothing: such a pair is evaluated at least 0.003 away
        spread = max(d["eval_spread"], 0.003) if s == t else d["eval_spread"]
        states.append(base + rs.normal(0, spread, 6))
    if d["eval_edge"] is not None:
        states[-1] = np.array(_edge_states()[d["eval_edge"]], dtype=np.float64)
    if d["motion"] is not None:                     # (`angles`: the drawn start, a sin / cos branch per axis)
        states[0] = np.array(d["init"], dtype=np.float64)
    if d["kind"] == "affine":
        a, b = d["illum"]
        states = [np.concatenate([x, ab]) for x, ab in zip(states, ((a, b), (0.0, 0.0), (-a, -b)))]
    return dict(gray=gray, depth=depth, K=K, pairs=run, states=np.array(states))


def run_device_sampled(d):
    """The device's side of a `sampled` case: every level evaluated at up to 3 (src, tgt, state), the pairs beyond them
    replicas; the planes of every level and frame as the device holds them."""
    from phovo_amd import native, odometry
    q = render_sequence(d)
    w, h, nl, n_pairs, nf = d["w"], d["h"], d["nl"], d["n_pairs"], d["n_frames"]
    with odometry.AlignmentEngine(0) as e:
        e.set_config(native.make_config(num_levels=nl, max_iter=[1] * nl, min_grad=[0.0] * nl))
        if d["kind"] == "affine":
            e.set_objective(native.OBJECTIVE_PHOTOMETRIC_AFFINE)
        else:
            e.set_extensions(native.make_extensions(plane_storage=[native.STORAGE_F64, native.STORAGE_F32,
                                                                   native.STORAGE_F16][d["storage"]],
                                                    huber_delta=d["huber"], sampling=native.SAMPLING_BILINEAR,
                                                    jacobian_corrected=d["kind"] == "corrected"))
        e.set_build_all_levels(True)
        e.set_intrinsic_matrix(q["K"])
        e.set_depth_range(*d["upload_range"])
        e.reserve_frames(nf, w, h)
        for f in range(nf):
            e.upload_frame(f, q["gray"][f], q["depth"][f])
        e.set_depth_range(*d["range"])
        planes = [[e.get_level_planes(f, l) for f in range(nf)] for l in range(nl)]      # [level][frame] (i, d, gx, gy)
        m = len(q["pairs"])
        src = [q["pairs"][i % m][0] for i in range(n_pairs)]
        tgt = [q["pairs"][i % m][1] for i in range(n_pairs)]
        st = np.array([q["states"][i % m] for i in range(n_pairs)])
        out, geos = [], set()
        for l in range(nl):
            r = e.evaluate_sampled_pairs(src, tgt, st, l, want_structs=True)
            recs = [bytes(memoryview(x)) for x in r.pop("structs")]
            r["replicas_alike"] = [k for k in range(m, n_pairs) if recs[k] != recs[k % m]]
            out.append({k: (v[:m] if isinstance(v, np.ndarray) else v) for k, v in r.items()})
            geos.add(predicted_geometry("eval", planes[l][0][0].size))
    return dict(d=d, K=q["K"], pairs=q["pairs"], states=q["states"], planes=planes, out=out), geos


def sampled_reference(d, planes_l, level, K, pair, state):
    """(rows, H, g, cost) of sampled_system_ref on the planes of one level ([frame] (i, d, gx, gy)) for one pair."""
    import sampled_system_ref as ssr
    s, t = pair
    pl = (planes_l[s][0], planes_l[s][1], planes_l[t][0], planes_l[t][2], planes_l[t][3])
    lo, hi = d["range"]
    if d["kind"] == "affine":
        H, g, cost, rows = ssr.system8(pl, level, K, state, lo, hi)
    else:
        delta = None if d["huber"] is None else d["huber"][level]
        H, g, cost, rows = ssr.system6(pl, level, K, state, d["kind"] == "corrected", delta, lo, hi)
    return rows, H, g, cost


def _one_ulp_of_fx(K):
    K1 = np.array(K, dtype=np.float64)
    K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
    return K1


def _check_sampled(job):
    """sampled_system_ref.system6 / system8 under sampled_system_ref.check_against; rows == 0: the all-zero record with
    RANK_DEFICIENT; 0 < rows < dim: the flag and the values.  A miss is set aside under `eval`'s rule only."""
    import sampled_system_ref as ssr
    d, K = job["d"], job["K"]
    dim = 8 if d["kind"] == "affine" else 6
    worst, knife, info = 0.0, [], dict(systems=0, empty=0, deficient=0)
    for level, out in enumerate(job["out"]):
        if out["replicas_alike"]:
            return _ok("fail", np.inf, f"level {level}: replicas {out['replicas_alike'][:5]} differ from their originals")
        for i, (pair, state) in enumerate(zip(job["pairs"], job["states"])):
            ref = sampled_reference(d, job["planes"][level], level, K, pair, state)
            rows = ref[0]
            info["systems"] += 1
            info["empty"] += int(rows == 0)
            info["deficient"] += int(0 < rows < dim)
            got = (out["information"][i], out["gradient"][i], int(out["rows"][i]), float(out["cost"][i]))
            flags = int(out["flags"][i])
            ratio = _eval_ratio(got, ref)
            try:
                if rows == 0:
                    assert got[2] == 0 and not got[0].any() and not got[1].any() and got[3] == 0.0, ("empty", got[2])
                    assert flags == PAIR_RANK_DEFICIENT, ("flags", flags)
                else:
                    ssr.check_against(got[0], got[1], got[2], got[3], ref[1], ref[2], rows, ref[3])
                    finite = np.all(np.isfinite(ref[1])) and np.all(np.isfinite(ref[2])) and np.isfinite(ref[3])
                    want = (PAIR_RANK_DEFICIENT if rows < dim else 0) | (0 if finite else PAIR_NONFINITE)
                    assert flags == want, ("flags", flags, want)
                worst = max(worst, ratio)
            except AssertionError as err:
                ref1 = sampled_reference(d, job["planes"][level], level, _one_ulp_of_fx(K), pair, state)
                moved = _eval_ratio((ref1[1], ref1[2], ref1[0], ref1[3]), ref)
                detail = (f"level {level} state {i} pair {pair}: {err}; rows {got[2]} / {rows}, distance / bar {ratio:.3g}, "
                          f"one ulp of fx moves the checker {moved:.3g} bars")
                if moved <= 0.25:
                    return dict(_ok("fail", ratio, detail), info=info)
                knife.append(detail)                  # (and the remaining levels and states are still checked)
    return dict(_ok("skip", worst, "; ".join(knife)) if knife else _ok("ok", worst), info=info)


def precheck_sampled(d):
    """The checker's side of a `sampled` case alone, on oracle-built pyramids in place of the device's: per system its row
    count and whether it is unstable under the one-ulp question (its own answer moves by more than a quarter of the bar, or
    its row count changes).  Returns dict(systems, empty, deficient, unstable (cases: 0 or 1), worst_moved)."""
    from oracle import oracle
    q = render_sequence(d)
    nl, nf = d["nl"], d["n_frames"]
    ocfg = oracle.make_config(num_levels=nl, max_iter=[1] * nl, min_grad=[0.0] * nl)
    pyr = []
    for f in range(nf):
        i0p, d0p = oracle.build_source_pyramids(q["gray"][f], q["depth"][f], ocfg)
        i1p, gxp, gyp = oracle.build_target_pyramids(q["gray"][f], ocfg)
        pyr.append([(i1p[l], d0p[l], gxp[l], gyp[l]) for l in range(nl)])
    dim = 8 if d["kind"] == "affine" else 6
    out = dict(systems=0, empty=0, deficient=0, unstable=0, worst_moved=0.0)
    K1 = _one_ulp_of_fx(q["K"])
    for level in range(nl):
        planes_l = [pyr[f][level] for f in range(nf)]
        for pair, state in zip(q["pairs"], q["states"]):
            ref = sampled_reference(d, planes_l, level, q["K"], pair, state)
            ref1 = sampled_reference(d, planes_l, level, K1, pair, state)
            moved = _eval_ratio((ref1[1], ref1[2], ref1[0], ref1[3]), ref)
            out["systems"] += 1
            out["empty"] += int(ref[0] == 0)
            out["deficient"] += int(0 < ref[0] < dim)
            if moved > 0.25:
                out["unstable"] = 1
            elif ref[0] > 0:
                out["worst_moved"] = max(out["worst_moved"], float(moved))
    return out


def _tr_options(d, nl):
    """Per-level options: those of a shipped Ceres file (level L of the file, or its last level) or fixed mode (every
    tolerance and the minimum radius 0, the default radii)."""
    from phovo_amd import native
    if d["ceres"] == "fixed":
        src = native.trust_region_options_default()
    else:
        cfg, src = native.read_trust_region_file(os.path.join(TESTS, "golden", "ceres", d["ceres"]))
    opt = native.TrustRegionOptions()
    fields = native.TR_OPTION_FIELDS
    for f in fields:
        getattr(opt, f)[:] = getattr(src, f)[:]
    if d["ceres"] == "fixed":
        for L in range(nl):
            opt.function_tolerance[L] = opt.gradient_tolerance[L] = opt.parameter_tolerance[L] = 0.0
            opt.min_trust_region_radius[L] = 0.0
    else:
        last = cfg.num_levels - 1
        for L in range(last + 1, nl):
            for f in fields:
                getattr(opt, f)[L] = getattr(opt, f)[last]
    return opt, types.SimpleNamespace(**{f: list(getattr(opt, f)) for f in fields})


def _plain_report(r):
    return types.SimpleNamespace(flags=int(r.flags), iterations=list(r.iterations), valid_pixels=list(r.valid_pixels),
                                 gradient_norm=float(r.gradient_norm))


def run_device(d):
    """The device's side of one case; returns a job for check_job (plain, picklable data) and the geometries it ran."""
    from phovo_amd import native, odometry
    p = render(d)
    w, h, nl, n_pairs = d["w"], d["h"], d["nl"], d["n_pairs"]
    lo, hi = d["range"]
    ulo, uhi = d["upload_range"]
    job = dict(d=d, p=p)
    geos = set()
    mode = d["mode"]
    with odometry.AlignmentEngine(0) as e:
        if mode == "bi":
            e.set_config(native.make_config(num_levels=nl, max_iter=d["max_iter"], min_grad=d["min_grad"], lam=d["lam"]))
            e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
        elif mode == "tr":
            e.set_config(native.make_config(num_levels=nl, max_iter=d["tr_max_iter"], min_grad=[0.0] * nl))
            e.set_objective(native.OBJECTIVE_TRUST_REGION)
            opt, job["opt"] = _tr_options(d, nl)
            e.set_trust_region_options(opt)
            e.set_batch_invariant(True)
        elif mode == "affine":
            e.set_config(native.make_config(num_levels=nl, max_iter=d["max_iter"], min_grad=d["min_grad"], lam=d["lam"]))
            e.set_objective(native.OBJECTIVE_PHOTOMETRIC_AFFINE)
        else:
            e.set_config(native.make_config(num_levels=nl, max_iter=[1] * nl, min_grad=[0.0] * nl))
            e.set_extensions(native.make_extensions(plane_storage=[native.STORAGE_F64, native.STORAGE_F32,
                                                                   native.STORAGE_F16][d["storage"]],
                                                    huber_delta=d["huber"]))
            e.set_build_all_levels(True)
        e.set_intrinsic_matrix(p["K"])
        e.set_depth_range(ulo, uhi)
        e.reserve_frames(2, w, h)
        e.upload_frame(0, p["gray0"], p["depth0"], native.ROLE_SOURCE)
        e.upload_frame(1, p["gray1"], p["depth1"] if mode == "bi" else None, native.ROLE_TARGET)
        e.set_depth_range(lo, hi)
        if mode == "affine":
            # the planes as the device holds them, of every level that runs (odd sizes: tests/pyramid_exact.py pins them)
            pyr = []
            for l in range(nl):
                if d["max_iter"][l] <= 0:
                    pyr.append(None)
                    continue
                i0, d0, _, _ = e.get_level_planes(0, l)
                i1, _, gx, gy = e.get_level_planes(1, l)
                pyr.append((i0, d0, i1, gx, gy))
                geos.update((chunk_class(i0.size), "last_partial" if i0.size % 64 else "last_full"))
            inits = None if p["init"] is None else np.tile(p["init"], (n_pairs, 1))
            s, reps = e.align_pairs([0] * n_pairs, [1] * n_pairs, init_states=inits, want_reports=True)
            job.update(pyr=pyr, states=s, reps=[_plain_report(r) for r in reps], illum=e.fetch_illumination(n_pairs),
                       kinds=sorted({r["kind"] for r in e.last_launches()}))
        elif mode in ("bi", "tr"):
            inits = None if p["init"] is None else np.tile(p["init"], (n_pairs, 1))
            s, reps = e.align_pairs([0] * n_pairs, [1] * n_pairs, init_states=inits, want_reports=True)
            for r in e.last_launches():
                n = int(np.prod(level_size(w, h, r["levels"][0])))
                geos.add(f"lds{r['threads']}" if r["lds_bytes"] >= 4 * n else f"hbm{r['threads']}")
            job["states"] = s
            job["reps"] = [_plain_report(r) for r in reps]
            if mode == "tr":
                job["tr"] = e.trust_region_reports(n_pairs)
        else:
            planes = [[], [], [], [], []]
            for l in range(nl):
                i0, d0, _, _ = e.get_level_planes(0, l)
                i1, _, gx, gy = e.get_level_planes(1, l)
                for lst, a in zip(planes, (i0, d0, i1, gx, gy)):
                    lst.append(a)
            rs = np.random.RandomState(d["defect_seed"] + 1)
            m = min(3, n_pairs)
            base = np.array(p["motion"])
            states = [base + rs.normal(0, d["eval_spread"], 6) for _ in range(m)]
            if d["eval_edge"] is not None:
                states[-1] = _edge_states()[d["eval_edge"]]
            if p["init"] is not None and d["motion"] is not None:
                states[0] = p["init"]
            st = np.array([states[i % m] for i in range(n_pairs)])
            job["planes"], job["eval_states"], job["eval"] = planes, st[:m], []
            for l in range(nl):
                out = e.evaluate_pairs([0] * n_pairs, [1] * n_pairs, st, l)
                job["eval"].append(out)
                geos.add(predicted_geometry("eval", int(np.prod(level_size(w, h, l)))))
    return job, geos


def _ok(status, ratio, msg=""):
    return dict(status=status, ratio=ratio, msg=msg)


def check_job(job):
    """The checker's side of one case, in a worker process (no GPU): dict(status ok / fail / skip, ratio, msg)."""
    try:
        return {"bi": _check_bi, "tr": _check_tr, "eval": _check_eval, "affine": _check_affine,
                "sampled": _check_sampled}[job["d"]["mode"]](job)
    except Exception as ex:                                     # a checker that raises is a failure, with its reason
        import traceback
        return _ok("fail", np.inf, "checker raised: " + "".join(traceback.format_exception_only(type(ex), ex)).strip())


def _same_report(a, b):
    """Two reports alike, a NaN gradient norm (a NaN target depth makes the gain NaN) equal to itself."""
    return (a.flags == b.flags and a.iterations == b.iterations and a.valid_pixels == b.valid_pixels and
            np.array_equal(a.gradient_norm, b.gradient_norm, equal_nan=True))


def _tr_levels(tr, recs, nl):
    """Device record against the checker's, level by level (printed with a failure)."""
    out = []
    for L in sorted(recs):
        r = recs[L]
        out.append(f"L{L}: steps {tr['steps'][0, L]}/{r['steps']} accepted {tr['accepted'][0, L]}/{r['accepted']} "
                   f"term {tr['termination'][0, L]}/{r['termination']} rows {tr['rows'][0, L]}/{r['rows']} "
                   f"cost {tr['initial_cost'][0, L]:.17g}/{r['initial_cost']:.17g} -> {tr['final_cost'][0, L]:.17g}/"
                   f"{r['final_cost']:.17g} radius {tr['final_radius'][0, L]:.17g}/{r['final_radius']:.17g} "
                   f"noise_from {r['noise_from']} min_rel_dc {r['min_rel_dc']:.2e} "
                   f"margin {min(r['margins'], default=1.0):.2e} decisions {r['decisions'][-6:]}")
    return "; ".join(out)


def _check_bi(job):
    from oracle import oracle
    from test_gpu_objective_edges import BiExpect
    d, p = job["d"], job["p"]
    nl = d["nl"]
    ocfg = oracle.make_config(num_levels=nl, max_iter=d["max_iter"], min_grad=d["min_grad"], lam=d["lam"])
    ex = BiExpect(ocfg, p, p["init"], d["range"][0], d["range"][1], d["upload_range"][1], guard=False)
    s, reps = job["states"], job["reps"]
    for k in range(1, len(reps)):
        if not (np.array_equal(s[k], s[0], equal_nan=True) and _same_report(reps[k], reps[0])):
            return _ok("fail", np.inf, f"replica {k} differs from replica 0")
    ratio = 0.0
    if ex.finite and np.all(np.isfinite(s[0])):
        from phovo_amd import se3
        ratio = se3.state_distance(s[0], ex.state) / ex.bar
    try:
        ex.check(s[0], reps[0], "pair 0")
        return _ok("ok", ratio)
    except AssertionError as err:
        sens = ex.sensitivity() if ex.finite else 0.0
        detail = f"{err}; cond {ex.cond:.2e} bar {ex.bar:.1e} one-ulp sensitivity {sens:.2e}"
        if sens > 0.25 * ex.bar:
            return _ok("skip", ratio, detail)
        return _ok("fail", ratio, detail)


def _check_tr(job):
    import test_gpu_trust_region as gtr
    import trust_region_ref as tref
    from oracle import oracle
    d, p = job["d"], job["p"]
    nl = d["nl"]
    ocfg = oracle.make_config(num_levels=nl, max_iter=d["tr_max_iter"], min_grad=[0.0] * nl)
    xs, recs = tref.align(ocfg, p["K"], p["gray0"], p["depth0"], p["gray1"], job["opt"], p["init"], *d["range"])
    s, tr = job["states"], job["tr"]
    for k in range(1, len(s)):
        if not (np.array_equal(s[k], s[0], equal_nan=True) and tr[k:k + 1].tobytes() == tr[0:1].tobytes()):
            return _ok("fail", np.inf, f"replica {k} differs from replica 0")
    margin = min((min(r["margins"], default=1.0) for r in recs.values()), default=1.0)
    if margin <= gtr.MARGIN:
        return _ok("skip", 0.0, f"decision margin {margin:.2e}")
    try:
        return _ok("ok", gtr.compare_pair(0, s[0], job["reps"][0], tr, xs, recs, nl, relative_pose=True))
    except AssertionError as err:
        strict = err
    # _check's bars hold the pose to 1e-9 x max(1, |x|) whatever the conditioning; as for `bi` (BiExpect), the pose bar
    # scales with cond(J^T J) of the checker's systems above 1e5 and the cost, Jacobi-scaling and gradient-norm bars take
    # what that pose bar carries into them to first order.  Decisions, rows and flags are still compared exactly.
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    allow = conditioned_allowance(recs, xs, lambda L, x: tref.evaluate(i0p[L], d0p[L], i1p[L], gxp[L], gyp[L], L, p["K"], x,
                                                                          *d["range"]))
    try:
        return _ok("conditioned", gtr.compare_pair(0, s[0], job["reps"][0], tr, xs, recs, nl, relative_pose=True,
                                                   allow=allow), f"{strict}; cond {allow['cond']:.2e}")
    except AssertionError as err:
        detail = f"{err}; cond {allow['cond']:.2e}, pose bar {allow['pose']:.1e}; device / checker {_tr_levels(tr, recs, nl)}"
        return _ok("fail", np.inf, detail)


def conditioned_allowance(recs, xs, evaluate_at):
    """Bars of a trust-region comparison conditioned on the checker's systems: the pose bar 1e-9 x max(1, cond / 1e5),
    capped at 1e-5, times max(1, |x|) (cond: the largest cond(J^T J) of the states the checker accepted, inf where fewer
    than six rows constrain it); what a pose difference e of that size adds to a cost (|g| |e| + |H| |e|^2 / 2), to a
    level's Jacobi scaling (summed one-coordinate differences of S at the level's entering state; 0 on the first level,
    which starts from the same state on both sides), to its final radius (through rho on every accepted step) and to the
    gradient norm (|H| |e|).  evaluate_at(level, x) is the
    checker's evaluation."""
    from test_gpu_trust_region import POSE_TOL
    cond = max(r["cond"] for r in recs.values())
    pose = min(1e-5, POSE_TOL * max(1.0, cond / 1e5)) * max(1.0, float(np.abs(xs).max()))
    e = np.sqrt(6.0) * pose
    allow = dict(cond=cond, pose=pose)
    first = max(recs)
    for L, r in recs.items():
        h2 = float(np.linalg.norm(r["H"], 2)) if np.all(np.isfinite(r["H"])) else np.inf
        allow[(L, "initial_cost")] = float(np.linalg.norm(r["g0"])) * e + 0.5 * h2 * e * e
        allow[(L, "final_cost")] = float(np.linalg.norm(r["g"])) * e + 0.5 * h2 * e * e
        # the radius: each accepted step multiplies it by 1 / max(1/3, 1 - (2 rho - 1)^3), whose logarithmic derivative
        # in rho is at most 6 x 0.763 / (1/3) = 13.7; rho = dc / mcc moves by at most 2 x (cost bar) / |dc|, and
        # |dc| >= min_rel_dc x final cost on every accepted step
        dc_min = r["min_rel_dc"] * r["final_cost"] if np.isfinite(r["min_rel_dc"]) else np.inf
        cost_bar = max(allow[(L, "initial_cost")], allow[(L, "final_cost")])
        allow[(L, "radius")] = (13.7 * r["accepted"] * 2.0 * cost_bar / dc_min if dc_min > 0 else np.inf) if r["accepted"] else 0.0
        if L != first:
            S0 = 1.0 / (1.0 + np.sqrt(np.diag(evaluate_at(L, r["x0"])["H"])))
            dS = np.zeros(6)
            for k in range(6):
                x = np.array(r["x0"], dtype=np.float64)
                x[k] += pose
                dS += np.abs(1.0 / (1.0 + np.sqrt(np.diag(evaluate_at(L, x)["H"]))) - S0)
            allow[(L, "S")] = dS
    last = recs[min(recs)]
    allow["gradient_norm"] = (float(np.linalg.norm(last["H"], 2)) if np.all(np.isfinite(last["H"])) else np.inf) * e
    return allow


def _eval_reference(planes, level, K, st, delta, lo, hi):
    from test_gpu_pair_system import _numpy_system, _oracle_trace_system
    rows, H, g = _oracle_trace_system(planes, level, K, st, delta, lo, hi)
    _, _, cost = _numpy_system(planes, level, K, st, delta, lo, hi)
    return rows, H, g, cost


def _eval_ratio(got, ref):
    """Distance / bar of a device system (H, g, rows, cost) from a reference, under test_gpu_pair_system's bars."""
    H, g, rows, cost = got
    rrows, rH, rg, rcost = ref
    if rows != rrows:
        return np.inf
    if rrows == 0:
        return 0.0 if not np.any(H) else np.inf
    scale = np.max(np.abs(rH))
    gbar = 1e-9 * np.sqrt(np.maximum(np.diag(rH) * rcost, 0.0))
    with np.errstate(all="ignore"):
        rg_ = np.max(np.where(gbar > 0, np.abs(g - rg) / gbar, np.where(g == rg, 0.0, np.inf)))
    return max(np.max(np.abs(H - rH)) / (1e-10 * scale) if scale > 0 else 0.0, rg_,
               abs(cost - rcost) / (1e-12 * abs(rcost)) if rcost != 0 else float(cost != 0))


def _check_eval(job):
    from test_gpu_pair_system import _check_against
    d, p = job["d"], job["p"]
    lo, hi = d["range"]
    K, planes, states = p["K"], job["planes"], job["eval_states"]
    m, worst, knife = len(states), 0.0, []
    for level, out in enumerate(job["eval"]):
        n = len(out["rows"])
        for k in range(m, n):
            j = k % m
            if not (np.array_equal(out["information"][k], out["information"][j]) and
                    np.array_equal(out["gradient"][k], out["gradient"][j]) and out["cost"][k] == out["cost"][j] and
                    out["rows"][k] == out["rows"][j]):
                return _ok("fail", np.inf, f"level {level}: replica {k} differs from {j}")
        delta = None if d["huber"] is None else d["huber"][level]
        for i in range(m):
            ref = _eval_reference(planes, level, K, states[i], delta, lo, hi)
            got = (out["information"][i], out["gradient"][i], int(out["rows"][i]), float(out["cost"][i]))
            ratio = _eval_ratio(got, ref)
            try:
                if ref[0] == 0:
                    assert got[2] == 0 and not np.any(got[0]), (got[2], ref[0])
                else:
                    _check_against(got[0], got[1], got[2], got[3], ref[1], ref[2], ref[0], ref[3])
                worst = max(worst, ratio)
            except AssertionError as err:
                K1 = K.copy()
                K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
                ref1 = _eval_reference(planes, level, K1, states[i], delta, lo, hi)
                moved = _eval_ratio((ref1[1], ref1[2], ref1[0], ref1[3]), ref)
                detail = f"level {level} state {i}: {err}; distance / bar {ratio:.3g}, one ulp of fx moves the oracle {moved:.3g} bars"
                if moved <= 0.25:
                    return _ok("fail", ratio, detail)
                knife.append(detail)                  # (and the remaining levels and states are still checked)
    return _ok("skip", worst, "; ".join(knife)) if knife else _ok("ok", worst)


def affine_reference(d, K, pyr, init):
    """affine_ref.optimize on the case's planes under its configuration and the depth range in force at the alignment."""
    import affine_ref as ar
    nl = d["nl"]
    cfg = dict(num_levels=nl, lam=d["lam"], max_iter=d["max_iter"], min_grad=d["min_grad"], min_depth=d["range"][0],
               max_depth=d["range"][1])
    return ar.optimize(pyr, K, cfg, init)


def affine_outcome(d, ref):
    """What the summary counts, from the checker's result alone: finite or not, flat or scaled bar, and of the levels that
    ran under a gradient threshold how many ended by it and how many by their iteration count."""
    import affine_ref as ar
    finite = bool(np.all(np.isfinite(ref["state"])))
    bar = ar.pose_bar(ref["cond"], ref["state"]) if finite else np.nan
    big = max(1.0, float(np.abs(ref["state"]).max())) if finite else np.nan
    thr = cnt = 0
    for L in range(d["nl"]):
        if d["max_iter"][L] > 0 and d["min_grad"][L] > 0 and finite:
            thr += int(ref["iterations"][L] < d["max_iter"][L])
            cnt += int(ref["iterations"][L] >= d["max_iter"][L])
    return dict(finite=finite, bar=bar, scaled=finite and bar > 1e-9 * big, capped=finite and bar >= 1e-5 * big,
                by_threshold=thr, by_count=cnt, no_rows=not finite and sum(ref["valid_pixels"]) == 0)


def affine_unstable(d, K, pyr, init, ref):
    """The knife-edge question: does one ulp of fx change the checker's own counts, flags or finiteness, or move its state
    by more than a quarter of the bar?  Returns (unstable, why)."""
    import affine_ref as ar
    K1 = np.array(K, dtype=np.float64)
    K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
    ref1 = affine_reference(d, K1, pyr, init)
    fin, fin1 = np.isfinite(ref["state"]), np.isfinite(ref1["state"])
    if (ref1["iterations"] != ref["iterations"] or ref1["valid_pixels"] != ref["valid_pixels"] or
            ref1["flags"] != ref["flags"] or not np.array_equal(fin, fin1)):
        return True, (f"one ulp of fx changes the checker's counts: iterations {ref['iterations']} -> {ref1['iterations']}, "
                      f"rows {ref['valid_pixels']} -> {ref1['valid_pixels']}, flags {ref['flags']} -> {ref1['flags']}")
    if not np.all(fin):
        return False, "one ulp of fx leaves the checker's counts and non-finite entries as they are"
    moved = float(np.abs(ref1["state"] - ref["state"]).max())
    bar = ar.pose_bar(ref["cond"], ref["state"])
    return moved > 0.25 * bar, f"one ulp of fx moves the checker's state by {moved:.2e} (bar {bar:.1e})"


def precheck_affine(d):
    """The checker's side of an `affine` case on oracle-built pyramids in place of the device's (DESIGN.md §3.6 has them
    bit-identical), for the CPU pre-check of the committed sweeps: affine_outcome's counts, whether the case is unstable
    under the one-ulp question, whether it comes within MARGIN_FLOOR of a threshold, whether it meets a system of 1-7 rows."""
    from oracle import oracle
    p = render(d)
    nl = d["nl"]
    ocfg = oracle.make_config(num_levels=nl, max_iter=[1] * nl, min_grad=[0.0] * nl)
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    pyr = [(i0p[l], d0p[l], i1p[l], gxp[l], gyp[l]) for l in range(nl)]
    ref = affine_reference(d, p["K"], pyr, p["init"])
    out = affine_outcome(d, ref)
    out["unstable"] = affine_unstable(d, p["K"], pyr, p["init"], ref)[0]
    out["near_threshold"] = bool(ref["margin"] <= MARGIN_FLOOR)
    out["noise"] = ref["noise_level"] is not None
    return out


def _check_affine(job):
    import affine_ref as ar
    d, p = job["d"], job["p"]
    nl = d["nl"]
    if job["kinds"] != ["affine"]:
        return _ok("fail", np.inf, f"launch kinds {job['kinds']}")
    s, ab, reps = job["states"], job["illum"], job["reps"]
    for k in range(1, len(reps)):
        if not (np.array_equal(s[k], s[0], equal_nan=True) and np.array_equal(ab[k], ab[0], equal_nan=True) and
                _same_report(reps[k], reps[0])):
            return _ok("fail", np.inf, f"replica {k} differs from replica 0")
    ref = affine_reference(d, p["K"], job["pyr"], p["init"])
    info = affine_outcome(d, ref)
    if ref["margin"] <= MARGIN_FLOOR:
        return dict(_ok("skip", 0.0, f"threshold margin {ref['margin']:.2e}: not compared"), info=info)
    dev, rep = np.concatenate([s[0], ab[0]]), reps[0]
    ratio, bar = 0.0, info["bar"]
    try:
        assert list(rep.iterations[:nl]) == ref["iterations"], ("iterations", rep.iterations[:nl], ref["iterations"])
        assert list(rep.valid_pixels[:nl]) == ref["valid_pixels"], ("rows", rep.valid_pixels[:nl], ref["valid_pixels"])
        assert rep.flags == ref["flags"], ("flags", rep.flags, ref["flags"])
        if not info["finite"]:
            bad = ~np.isfinite(ref["state"])
            assert not np.any(np.isfinite(dev[bad])), ("finite where the checker is not", dev, ref["state"])
        else:
            ratio = float(np.abs(dev - ref["state"]).max()) / bar if np.all(np.isfinite(dev)) else np.inf
            assert ratio <= 1.0, ("state", dev, ref["state"])
            gbar = 1e-9 * max(1.0, ref["gradient_norm"])
            if info["scaled"]:                      # what the scaled pose bar carries into the gradient, to first order
                gbar += ref["h_norm"] * np.sqrt(8.0) * bar
            assert abs(rep.gradient_norm - ref["gradient_norm"]) <= gbar, ("gradient norm", rep.gradient_norm,
                                                                           ref["gradient_norm"], gbar)
        return dict(_ok("ok", ratio), info=info)
    except AssertionError as err:
        noise = ref["noise_level"]
        if noise is not None:
            # a system of 1 ... 7 rows on level `noise`: its step is rounding noise on both sides and no
            # report after it is defined.  What is: the flag, and the levels that ran before.  Counted as set aside.
            before = [L for L in range(noise + 1, nl) if d["max_iter"][L] > 0]
            if (rep.flags & ar.PAIR_RANK_DEFICIENT and all(rep.iterations[L] == ref["iterations"][L] and
                                                           rep.valid_pixels[L] == ref["valid_pixels"][L] for L in before)):
                return dict(_ok("skip", 0.0, f"{err}; undefined after a system of 1-7 rows on level {noise}: "
                                             f"RANK_DEFICIENT set, levels {before} alike"), info=info)
        unstable, why = affine_unstable(d, p["K"], job["pyr"], p["init"], ref)
        detail = (f"{err}; device it {list(rep.iterations[:nl])} rows {list(rep.valid_pixels[:nl])} flags {rep.flags} "
                  f"state {dev.tolist()}; checker {ref['iterations']} {ref['valid_pixels']} {ref['flags']} "
                  f"{ref['state'].tolist()} cond {ref['cond']:.2e} bar {bar:.1e} distance / bar {ratio:.3g}; {why}")
        return dict(_ok("skip" if unstable else "fail", ratio, detail), info=info)


def main(argv):
    import concurrent.futures as cf
    import multiprocessing as mp
    cases = int(argv[1]) if len(argv) > 1 else 100
    seed = int(argv[2]) if len(argv) > 2 else 0
    mode = argv[3] if len(argv) > 3 else "bi"
    if mode not in MODES:
        raise SystemExit(f"mode must be one of {MODES}")
    flags = set(argv[4:])
    only = {int(c) for c in os.environ["FUZZ_ONLY"].split(",")} if os.environ.get("FUZZ_ONLY") else None
    draws = draw_cases(cases, seed, mode, flags, only)

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import _variant
    _variant.use_from_environment()       # PHOVO_TOOLS_LIBRARY=<another build>: sweep that build instead (tools/_variant.py)
    import phovo_amd  # noqa: F401

    jobs = int(os.environ.get("FUZZ_JOBS", min(12, os.cpu_count() or 1)))
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = "1"                 # (inherited by the workers: one thread each)
    bad = skipped = done = conditioned = 0
    worst, geos, pending = 0.0, {}, []
    tally = dict(scaled=0, nonfinite=0, by_threshold=0, by_count=0)          # (affine, from the checker's results)
    systems = dict(systems=0, empty=0, deficient=0)                          # (sampled, from the checker's results)

    def settle(fut, case, d):
        nonlocal bad, skipped, done, worst, conditioned
        r = fut.result()
        done += 1
        desc = (f"case {case}: {d['w']}x{d['h']} levels {d['nl']} pairs {d['n_pairs']} range {d['range']} upload "
                f"{d['upload_range']} src {d['src_defects']} tgt {d['tgt_defects']}")
        if mode == "affine":
            desc += f" max_iter {d['max_iter']} min_grad {d['min_grad']} lam {d['lam']} exposure {d['exposure']}"
            if "info" in r:
                i = r["info"]
                tally["scaled"] += int(r["status"] == "ok" and i["scaled"])
                tally["nonfinite"] += int(not i["finite"])
                tally["by_threshold"] += i["by_threshold"]
                tally["by_count"] += i["by_count"]
        if mode == "sampled":
            desc += (f" kind {d['kind']} storage {d['storage']} huber {d['huber']} frames {d['n_frames']} "
                     f"(src, tgt) {sampled_pairs_run(d)} sparse {d['sparse']} k_perturb {d['k_perturb']}")
            for k in systems:
                systems[k] += r.get("info", {}).get(k, 0)
        if r["status"] == "fail":
            bad += 1
            print(f"FAIL {desc}: {r['msg']}", flush=True)
        elif r["status"] == "skip":
            skipped += 1
            print(f"knife-edge {desc}: {r['msg']}", flush=True)
        else:
            worst = max(worst, r["ratio"])
            conditioned += int(r["status"] == "conditioned")
        if done % 100 == 0:
            print(f"... {done} cases so far, {bad} failures, {skipped} skipped", flush=True)

    with cf.ProcessPoolExecutor(max_workers=jobs, mp_context=mp.get_context("spawn")) as pool:
        for case, d in draws.items():
            job, g = run_device_sampled(d) if mode == "sampled" else run_device(d)
            for x in g:
                geos[x] = geos.get(x, 0) + 1
            pending.append((pool.submit(check_job, job), case, d))
            while len(pending) > 3 * jobs:
                settle(*pending.pop(0))
        for item in pending:
            settle(*item)
    n = len(draws)
    print(f"{n} cases, {bad} failures, {skipped} skipped as knife-edge, worst distance / bar {worst:.3f}"
          + (f"; {conditioned} passed only under the bars conditioned on cond(J^T J)" if mode == "tr" else "")
          + (f"; {tally['scaled']} passed only under the scaled bar, {tally['nonfinite']} ended non-finite; levels under a "
             f"threshold ended by threshold: {tally['by_threshold']}, by count: {tally['by_count']}" if mode == "affine" else "")
          + (f"; {systems['systems']} systems checked, {systems['empty']} empty, {systems['deficient']} of fewer rows than "
             f"columns" if mode == "sampled" else ""))
    if mode == "sampled":
        print("coverage (sampled, of the draws run): " + ", ".join(f"{k}: {v}" for k, v in coverage_sampled(draws.values()).items()))
    what = ("tile classes predicted from the level sizes" if mode == "eval" else
            "tile classes of the levels as the device sized them" if mode == "sampled" else
            "chunk classes of the levels run" if mode == "affine" else "from the launch records")
    print(f"geometries exercised ({mode}, {what}): " + ", ".join(f"{k}: {v}" for k, v in sorted(geos.items())))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
