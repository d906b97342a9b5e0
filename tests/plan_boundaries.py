"""Level sizes at which a launch geometry is taken for the first or the last time, shared by
tests/test_plan_boundaries_cpu.py (which vouches for them without a GPU) and tests/test_gpu_plan_boundaries.py (which runs
them).  Test infrastructure, not collected as tests.

Every aligner picks its kernel form from a level's pixel count n alone, by LDS sums: the fixed block, the owner map padded
to whole 64-pixel chunks plus one round of the workgroup's chunks, the ballot masks, and the depth park block, which takes
whatever is left.  The largest level a form accepts fills its LDS block to the last few bytes; there the park block holds
no chunk, one chunk or every chunk, and an off-by-one in a size, a pad, a round-up or a run selection shows first -- and
quietly: an LDS access past the block does not fault, reads give 0 and writes vanish.

This module holds
  * a restatement in Python of the four planning functions (gn_plan_level, gn_level_fusable, gn_plan_level_biobjective,
    gn_plan_level_trust_region), written from the constants of csrc/gn_device.hpp and the .hip files.  The GPU module
    compares the library's choice with it for every case: a planner constant that moves fails there, loudly, instead of
    turning a boundary case into an interior one;
  * the tables of shapes, derived by hand from those constants (c = ceil(n / 64) chunks);
  * the inputs and the CPU references of every case.
"""
import functools
import os

import numpy as np

import biobjective_ref as bref
import trust_region_ref as tref

import phovo_amd  # noqa: F401
from phovo_amd import native, se3, synthetic
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "config_files")
CERES_DIR = os.path.join(ROOT, "tests", "golden", "ceres")

POSE_TOL = 1e-9           # the project's bar (tests/test_gpu_parity.py); flat here: every case has cond(J^T J) < 1e5
COND_MAX = 1e5
GRAD_TOL = 1e-9           # gradient norm, relative
THRESHOLD_MARGIN = 0.005  # fused bases: no gradient norm of the oracle's trace within 0.5 % of a threshold

# ------------------------------------------------------------------------------------------------------------------------
# the planners, restated (csrc/gn_device.hpp, gn_kernels.hip, gn_biobjective_kernel.hip, gn_trust_region_kernel.hip)
# ------------------------------------------------------------------------------------------------------------------------
WAVE = 64
LDS_LIMIT = 160 * 1024
NRED = 32
CTL_COUNT = 4
TR_COUNT, TRI_COUNT = 50, 8
OWNER_INDEX_MASK = (1 << 21) - 1
CHUNK_BYTES = 8 * WAVE                 # one parked chunk: 64 doubles


def chunks(n):
    return (n + WAVE - 1) // WAVE


def lds_fixed_bytes(threads):
    """Pose constants [32], state [8], one row of NRED wave sums per wave (doubles), control words (ints)."""
    return 8 * (32 + 8 + (threads // WAVE) * NRED) + 4 * CTL_COUNT


def tr_lds_fixed_bytes(threads):
    return lds_fixed_bytes(threads) + 8 * TR_COUNT + 4 * TRI_COUNT


def owner_lds_entries(n, threads):
    """Whole chunks plus one round of the workgroup's chunks (pass 2 reads the owner a chunk ahead, unguarded)."""
    return ((n + 63) & ~63) + threads


def _plan(form, threads, wgs_per_cu, lds_bytes, parked=0, owner_in_lds=True, source_in_lds=False, seam=0,
          mask_in_hbm=False):
    return dict(form=form, threads=threads, wgs_per_cu=wgs_per_cu, lds_bytes=lds_bytes, parked=parked,
                owner_in_lds=owner_in_lds, source_in_lds=source_in_lds, owner_lds_entries=seam, mask_in_hbm=mask_in_hbm)


def _park(n, used, per_cu):
    """(lds_bytes, parked chunks): the leftover of LDS_LIMIT / per_cu behind `used` rounded up to 8, in 512-byte chunks."""
    used = (used + 7) & ~7
    room = LDS_LIMIT // per_cu
    parked = min((room - used) // CHUNK_BYTES if room > used else 0, chunks(n))
    return used + CHUNK_BYTES * parked, parked


def plan_level(n, prefer_latency=False, bound_by_bytes=True):
    """gn_plan_level.  bound_by_bytes: fp64 planes (what the engine passes); prefer_latency: a handful of pairs under
    phovo_engine_set_latency_forms.  None where the library refuses the level."""
    c = chunks(n)

    def owner_bytes(t):
        return 4 * owner_lds_entries(n, t)

    if n <= 2048 and not prefer_latency and c <= 64:
        lds, parked = _park(n, lds_fixed_bytes(64) + owner_bytes(64), 16)
        return _plan("SOLO", 64, 16, lds, parked)
    if n <= 2048:
        return _plan("TINY", 256, 4, lds_fixed_bytes(256) + owner_bytes(256) + 8 * n, source_in_lds=True)
    f256, f512, f1024 = lds_fixed_bytes(256), lds_fixed_bytes(512), lds_fixed_bytes(1024)
    if not prefer_latency and c <= 64 * 4 and f256 + owner_bytes(256) <= LDS_LIMIT // 4:
        lds, parked = _park(n, f256 + owner_bytes(256), 4)
        return _plan("QUAD", 256, 4, lds, parked)
    fits_wide = c <= 64 * 16 and f1024 + owner_bytes(1024) <= LDS_LIMIT
    if c <= 64 * 8 and f512 + owner_bytes(512) <= LDS_LIMIT // 2:
        lds, parked = _park(n, f512 + owner_bytes(512), 2)
        mid_parks_little = parked * 4 < c
        if not (mid_parks_little and fits_wide and not prefer_latency and bound_by_bytes):
            return _plan("MID", 512, 2, lds, parked)
    if fits_wide:
        lds, parked = _park(n, f1024 + owner_bytes(1024), 1)
        return _plan("WIDE", 1024, 1, lds, parked)
    if n > OWNER_INDEX_MASK:
        return None
    mask = 8 * c
    mask_in_hbm = f1024 + mask > LDS_LIMIT // 2
    if mask_in_hbm:
        mask = 0
    seam = min((LDS_LIMIT - f1024 - mask) // 4 // WAVE * WAVE, n // WAVE * WAVE)
    return _plan("HUGE", 1024, 1, f1024 + mask + 4 * seam, owner_in_lds=False, seam=seam, mask_in_hbm=mask_in_hbm)


def level_fusable(n):
    """gn_level_fusable: the 512-thread geometry with its owner map in half a CU's LDS."""
    return n > 2048 and chunks(n) <= 64 * 8 and lds_fixed_bytes(512) + 4 * owner_lds_entries(n, 512) <= LDS_LIMIT // 2


def fused_lds_bytes(n_max):
    return lds_fixed_bytes(512) + 4 * owner_lds_entries(n_max, 512)


def fused_parked(n_max, n):
    """Chunks of a level of n pixels parked in the tail of the owner map sized for n_max (gn_launch_fused)."""
    spare = owner_lds_entries(n_max, 512) - owner_lds_entries(n, 512)
    return min(spare * 4 // CHUNK_BYTES, chunks(n))


def _plan_objective(n, fixed):
    mask, owner = 8 * chunks(n), 4 * n
    if fixed(256) + mask + owner <= LDS_LIMIT // 2:
        return _plan("SMALL", 256, 2, fixed(256) + mask + owner)
    if fixed(512) + mask + owner <= LDS_LIMIT:
        return _plan("LARGE", 512, 1, fixed(512) + mask + owner)
    if n > OWNER_INDEX_MASK or fixed(512) + mask > LDS_LIMIT:
        return None
    return _plan("HBM", 512, 1, fixed(512) + mask, owner_in_lds=False)


def plan_biobjective(n):
    return _plan_objective(n, lds_fixed_bytes)


def plan_trust_region(n):
    return _plan_objective(n, tr_lds_fixed_bytes)


def expected_launches(ns, mode):
    """(kind, threads, lds_bytes) of a throughput enqueue on fp64 planes whose active levels, coarse to fine, have ns
    pixels and all carry a gradient threshold (engine.cpp, phovo_engine_enqueue_align): a run of two or more consecutive
    fusable levels is one fused launch (FUSION_AUTO) or one 512-thread launch per level (FUSION_SPLIT); every other level
    takes its own plan."""
    out, i = [], 0
    while i < len(ns):
        run = i
        while mode != native.FUSION_OFF and run < len(ns) and level_fusable(ns[run]):
            run += 1
        if run - i >= 2:
            if mode == native.FUSION_AUTO:
                out.append(("fused", 512, fused_lds_bytes(max(ns[i:run]))))
            else:
                out += [("persistent", 512, fused_lds_bytes(n)) for n in ns[i:run]]
            i = run
            continue
        p = plan_level(ns[i])
        out.append(("persistent", p["threads"], p["lds_bytes"]))
        i += 1
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------------
ALL = "all"
# Photometric, fp64 planes, throughput launch.  (w, h): form, threads, parked chunks (ALL, a count, or None: whatever the
# restatement gives), which neighbour the row is ("last": c + 1 chunks are not accepted in this form; "first": c - 1 chunks
# -- or, for the park-driven MID/WIDE switch, the row above -- take another one), fixed iteration counts.
# 1, 2 and 4 iterations at the zero-, one- and all-parked shapes: the first trip alone, one trip that reads the park block,
# several of them; 3 elsewhere.
PHOTO = {
    (64, 32): dict(form="SOLO", threads=64, parked=2, edge="last", iters=(3,)),
    (50, 41): dict(form="QUAD", threads=256, parked=ALL, edge="first", iters=(3,)),
    (128, 74): dict(form="QUAD", threads=256, parked=1, edge=None, iters=(1, 2, 4)),
    (120, 80): dict(form="QUAD", threads=256, parked=0, edge="last", iters=(1, 2, 4)),
    (97, 99): dict(form="MID", threads=512, parked=None, edge="first", iters=(3,)),
    (128, 100): dict(form="MID", threads=512, parked=51, edge="last", iters=(3,)),
    (134, 96): dict(form="WIDE", threads=1024, parked=ALL, edge="first", iters=(1, 2, 4)),
    (129, 100): dict(form="WIDE", threads=1024, parked=ALL, edge=None, iters=(1, 2, 4)),
    (112, 116): dict(form="WIDE", threads=1024, parked=201, edge=None, iters=(3,)),
    (202, 192): dict(form="WIDE", threads=1024, parked=0, edge="last", iters=(1, 2, 4)),
}
# beyond LDS: the exact kernel with its owner map in HBM (HUGE), behind the sliding-window kernel by default
BEYOND = (200, 194)               # first level beyond LDS; the LDS part of the owner map ends at 38 592, 208 pixels in HBM
BEYOND_SEAM = 38592
EXACT = {
    (928, 668): dict(mask_in_hbm=False, edge="last"),     # c = 9686: the last size with the ballots in LDS
    (800, 775): dict(mask_in_hbm=True, edge=None),        # c = 9688: ballots in HBM
}
EXACT_ITERS = 2
# fp32 planes (bound_by_bytes false): MID up to its LDS limit, which is also the fused launch's limit
NARROW = {
    (151, 128): dict(form="MID", threads=512, parked=0, edge="last", iters=(1, 2, 4)),
    (192, 101): dict(form="WIDE", threads=1024, parked=None, edge="first", iters=(3,)),
}
HUBER_DELTA = 0.05
# phovo_engine_set_latency_forms(1), wide policy -1, at most 8 pairs: prefer_latency skips SOLO and QUAD
LATENCY = {
    (64, 32): dict(form="TINY", threads=256, source_in_lds=True),
    (50, 41): dict(form="MID", threads=512, source_in_lds=False),
    (151, 128): dict(form="MID", threads=512, source_in_lds=False),
    (192, 101): dict(form="WIDE", threads=1024, source_in_lds=False),
}
# Fused runs: three levels, max_iter [0, 7, 11], thresholds [0, 120, 120], 300 copies of one pair.
# base: (level 1, level 2), fused launch expected, the oracle's iteration counts where the issue states them
FUSED_MAX_ITER, FUSED_MIN_GRAD, FUSED_COPIES = [0, 7, 11], [0.0, 120.0, 120.0], 300
FUSED = {
    (302, 256): dict(levels=((151, 128), (76, 64)), fused=True),      # the largest level exactly at the limit
    (384, 202): dict(levels=((192, 101), (96, 50)), fused=False),     # level 1 not fusable
    (200, 164): dict(levels=((100, 82), (50, 41)), fused=True),       # the smallest level in the first fusable chunk
    (256, 128): dict(levels=((128, 64), (64, 32)), fused=False),      # level 2 not fusable
}
# Bi-objective and trust region: (w, h): form, threads, LDS bytes where the table names them, the named neighbour
BI = {
    (160, 122): dict(form="SMALL", threads=256, lds_bytes=81880, neighbour=(161, 122)),
    (161, 122): dict(form="LARGE", threads=512, lds_bytes=None, neighbour=(160, 122)),
    (208, 188): dict(form="LARGE", threads=512, lds_bytes=163688, neighbour=(209, 188)),
    (209, 188): dict(form="HBM", threads=512, lds_bytes=None, neighbour=(208, 188)),
}
TR = {
    (192, 101): dict(form="SMALL", threads=256, lds_bytes=81784, neighbour=(193, 101)),
    (193, 101): dict(form="LARGE", threads=512, lds_bytes=None, neighbour=(192, 101)),
    (200, 195): dict(form="LARGE", threads=512, lds_bytes=163696, neighbour=(201, 195)),
    (201, 195): dict(form="HBM", threads=512, lds_bytes=None, neighbour=(200, 195)),
}
OBJECTIVE_ITERS = 3                # bi-objective: fixed iterations
# Trust region: ten steps from the initial state of test_gpu_trust_region.py::test_three_level_blur_and_tolerances, of
# which four are accepted and six rejected.  From the zero state the checker itself is not well-posed: the first
# evaluation puts every border pixel exactly on the in-bounds limit, one ulp of fx moves whole columns across it, and the
# fixture's full 50 steps carry that to 1e-3 in the pose; three steps from there are all rejected and move nothing.
TR_STEPS = 10
TR_INIT = (0.01, -0.01, 0.02, 0.005, -0.004, 0.003)
# an initial state that leaves the sliding window at once (an in-plane rotation, as tests/test_gpu_parity.py uses)
LEAVES_WINDOW = (0.0, 0.0, 0.0, 0.3, 0.0, 0.0)


def size_id(size):
    return f"{size[0]}x{size[1]}"


def parked_count(row, n):
    return chunks(n) if row["parked"] == ALL else row["parked"]


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def cfgs(max_iter, min_grad=None):
    nl = len(max_iter)
    kw = dict(num_levels=nl, blur=[0] * nl, grad_scale=[0.0625] * nl, lam=[1.0] * nl, max_iter=list(max_iter),
              min_grad=[0.0] * nl if min_grad is None else list(min_grad))
    return native.make_config(**kw), oracle.make_config(min_depth=0.3, max_depth=5.0, **kw)


@functools.lru_cache(maxsize=None)
def pair(w, h):
    """The pair of a single-level case (as tests/test_gpu_persistent_depth.py)."""
    return synthetic.make_pair(13, w, h, holes=0.03, trans=0.01 * w / 640, rot=0.004)


@functools.lru_cache(maxsize=None)
def fused_pair(w, h):
    return synthetic.make_pair(77, w, h, holes=0.02, trans=0.02 * w / 448, rot=0.01)


@functools.lru_cache(maxsize=None)
def bi_pair(w, h):
    """As tests/test_gpu_biobjective.py::test_parity_in_the_512_thread_lds_geometry."""
    return synthetic.make_pair(21, w, h, holes=0.03)


@functools.lru_cache(maxsize=None)
def tr_pair(w, h):
    """As tests/test_gpu_trust_region.py::test_200x150_level."""
    return synthetic.make_pair(7, w, h)


def bi_cfgs():
    n = native.read_config_file(os.path.join(CFG_DIR, "config_only_level_0_analytic.yml"))
    nl = n.num_levels
    kw = dict(num_levels=nl, blur=list(n.blur_filter_size[:nl]), grad_scale=list(n.image_gradients_scaling_factor[:nl]),
              lam=list(n.lambda_optimization_step[:nl]), max_iter=[OBJECTIVE_ITERS] + [0] * (nl - 1), min_grad=[0.0] * nl)
    return native.make_config(**kw), oracle.make_config(**kw)


def tr_cfg():
    """The shipped Ceres fixture of the level-0 configuration with TR_STEPS steps at most."""
    cfg, opt = native.read_trust_region_file(os.path.join(CERES_DIR, "config_only_level_0_ceres.yml"))
    cfg.max_num_iterations[0] = TR_STEPS
    return cfg, opt


def storage_planes(ocfg, p, storage):
    """The five one-level plane lists the device holds for pair p under `storage` (numpy's rounding, which is what the
    device stores: tests/extension_forms.py)."""
    import extension_forms as ef
    return ef.emulated_planes(ocfg, p, storage)


# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------
def _bump_fx(K):
    K1 = K.copy()
    K1[0, 0] = np.nextafter(K1[0, 0], 2.0 * K1[0, 0])
    return K1


def _cond(hessians):
    c = 1.0
    for h in hessians:
        if np.all(np.isfinite(h)) and np.any(h != 0.0):
            c = max(c, float(np.linalg.cond(h)))
    return c


class PhotoRef:
    """The oracle's result of one photometric case on the given plane lists: state, iteration counts, valid pixels of each
    level's last iteration, last gradient norm, the trace, the largest cond(J^T J) of it and the gradient norm of every
    iteration; nudged(): the same run with fx one ulp larger."""

    def __init__(self, ocfg, K, planes, init=None, huber=None):
        self._args = (ocfg, planes, init, huber)
        self.K = K
        self.nl = ocfg.num_levels
        self.state, self.its, tr = self._run(K, True)
        self.trace = tr
        self.valid = oracle.valid_pixels_per_level(tr, self.nl)
        self.gnorm = float(np.linalg.norm(tr[-1]["gradient"]))
        self.gnorms = [(e["level"], float(np.linalg.norm(e["gradient"]))) for e in tr]
        self.cond = _cond(e["hessian"] for e in tr)
        self.finite = bool(np.all(np.isfinite(self.state)))

    def _run(self, K, trace):
        ocfg, planes, init, huber = self._args
        return oracle.optimize(ocfg, K, *planes, init_state=init, want_trace=trace, huber_delta=huber)

    def nudged(self):
        """(distance the oracle's own result moves, its iteration counts) with fx one ulp larger."""
        s1, its1 = self._run(_bump_fx(self.K), False)
        return (se3.state_distance(self.state, s1) if np.all(np.isfinite(s1)) else np.inf), its1


def _pyramids(ocfg, p):
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    return i0p, d0p, i1p, gxp, gyp


@functools.lru_cache(maxsize=None)
def photo_ref(size, iters, init=None, storage=native.STORAGE_F64, huber=False):
    """One level of `size`, `iters` fixed iterations, from `init` (a tuple), on the planes `storage` holds, with or without
    Huber weights."""
    p = pair(*size)
    _, ocfg = cfgs([iters])
    planes = _pyramids(ocfg, p) if storage == native.STORAGE_F64 else storage_planes(ocfg, p, storage)
    return PhotoRef(ocfg, p["K"], planes, None if init is None else np.array(init), [HUBER_DELTA] if huber else None)


@functools.lru_cache(maxsize=None)
def fused_ref(base):
    p = fused_pair(*base)
    _, ocfg = cfgs(FUSED_MAX_ITER, FUSED_MIN_GRAD)
    return PhotoRef(ocfg, p["K"], _pyramids(ocfg, p))


class BiRef:
    """The bi-objective checker's result of one case (tests/biobjective_ref.py)."""

    def __init__(self, ocfg, p):
        self._args = (ocfg, oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg),
                      bref.target_planes(p["gray1"], p["depth1"], ocfg, 5.0))
        self.K = p["K"]
        self.state, self.its, self.valid, self.flags, tr = self._run(self.K)
        self.cond = _cond(t["H"] for t in tr)
        self.finite = bool(np.all(np.isfinite(self.state)))
        # the gradient of the last iteration (the checker does not keep it): the system at the state one iteration earlier
        assert ocfg.num_levels == 1 and self.its[0] == ocfg.max_num_iterations[0] >= 2
        ocfg.max_num_iterations[0] -= 1
        before_last = self._run(self.K)[0]
        ocfg.max_num_iterations[0] += 1
        (i0p, d0p), t = self._args[1:]
        _, g, _ = bref.normal_equations(i0p[0], d0p[0], t["i1"][0], t["d1"][0], t["gx"][0], t["gy"][0], t["dgx"][0],
                                        t["dgy"][0], t["gain"][0], 0, self.K, before_last, 0.3, 5.0)
        self.gnorm = float(np.linalg.norm(g))

    def _run(self, K):
        ocfg, src, tgt = self._args
        return bref.optimize(ocfg, K, src, tgt, None, 0.3, 5.0)

    def nudged(self):
        s1, its1 = self._run(_bump_fx(self.K))[:2]
        return (se3.state_distance(self.state, s1) if np.all(np.isfinite(s1)) else np.inf), its1


@functools.lru_cache(maxsize=None)
def bi_ref(size):
    return BiRef(bi_cfgs()[1], bi_pair(*size))


class TrRef:
    """The trust-region checker's result of one case (tests/trust_region_ref.py): the state and the per-level records that
    test_gpu_trust_region.compare_pair holds the device to."""

    def __init__(self, cfg, opt, p):
        ocfg = tref.oracle_config(cfg)
        self._args = (ocfg, oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg),
                      oracle.build_target_pyramids(p["gray1"], ocfg), opt)
        self.K = p["K"]
        self.state, self.recs = self._run(self.K)
        self.its = {L: r["steps"] for L, r in self.recs.items()}
        self.cond = max(r["cond"] for r in self.recs.values())
        self.margin = min(min(r["margins"], default=1.0) for r in self.recs.values())
        self.finite = bool(np.all(np.isfinite(self.state)))

    def _run(self, K):
        ocfg, src, tgt, opt = self._args
        return tref.optimize(ocfg, K, src, tgt, opt, np.array(TR_INIT))

    def nudged(self):
        s1, recs1 = self._run(_bump_fx(self.K))
        its1 = {L: r["steps"] for L, r in recs1.items()}
        return (se3.state_distance(self.state, s1) if np.all(np.isfinite(s1)) else np.inf), its1


@functools.lru_cache(maxsize=None)
def tr_ref(size):
    cfg, opt = tr_cfg()
    return TrRef(cfg, opt, tr_pair(*size))
