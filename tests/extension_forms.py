"""Deterministic inputs of tests/test_gpu_extension_forms.py, shared with their CPU pre-checks in
tests/test_extensions_cpu.py.  Test infrastructure, not collected as tests.

Every input is a function of constants in this file, so the CPU pre-check vouches for exactly what the GPU module runs:
the oracle on the planes a narrow storage would hold (numpy's rounding, which is what the device stores:
test_narrow_storage_rounds_once_and_matches_oracle) is finite, well-posed for the project's pose bar (Expect's guard) and,
with Huber weights, has residuals beyond delta.
"""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import native, se3, synthetic
from oracle import oracle
from test_gpu_large_rotations import Expect

STORAGES = [native.STORAGE_F32, native.STORAGE_F16]
STORAGE_IDS = {native.STORAGE_F64: "f64", native.STORAGE_F32: "f32", native.STORAGE_F16: "f16"}
N_BATCH = 640                    # >= 512 pairs: one work queue per XCD
DELTA = 0.05                     # Huber delta of every active level; the occluder block's residuals are ~0.5
F16_MIN_NORMAL = 6.103515625e-05
STRIPS = [(1, 40), (2, 33), (3, 17), (4, 64), (5, 70), (75, 53)]


def round_image(a, storage):
    """An intensity / gradient plane as `storage` holds it (fp16 goes through fp32), as fp64."""
    if storage == native.STORAGE_F64:
        return np.asarray(a, dtype=np.float64)
    a = np.asarray(a).astype(np.float32)
    return (a.astype(np.float16) if storage == native.STORAGE_F16 else a).astype(np.float64)


def round_depth(a, storage):
    """A depth plane as `storage` holds it: fp32 under both narrow storages."""
    a = np.asarray(a, dtype=np.float64)
    return a if storage == native.STORAGE_F64 else a.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# forms of the scatter path: (size, max_iter, min_grad, settings, launches of a batch)
# a launch: (kind, threads, owner map in LDS, level of the launch whose pixel count the LDS test uses)
# ------------------------------------------------------------------------------------------------------------------------
def _form(size, max_iter, launches, min_grad=None, **settings):
    return dict(size=size, max_iter=max_iter, min_grad=min_grad or [0.0] * len(max_iter), launches=launches,
                settings=settings)


FORMS = {
    "threads64_40x30": _form((40, 30), [4], [("persistent", 64, True, 0)]),
    "threads256_80x60": _form((80, 60), [5], [("persistent", 256, True, 0)]),
    "threads512_128x96": _form((128, 96), [5], [("persistent", 512, True, 0)]),
    # (narrow planes: two workgroups of 512 per CU; fp64 planes take one of 1024 at this size)
    "threads512x2_160x120": _form((160, 120), [5], [("persistent", 512, True, 0)]),
    "threads1024_200x152": _form((200, 152), [4], [("persistent", 1024, True, 0)]),
    "latency256_40x30": _form((40, 30), [4], [("persistent", 256, True, 0)], latency=True),
    "latency512_80x60": _form((80, 60), [5], [("persistent", 512, True, 0)], latency=True),
    "fused_320x240": _form((320, 240), [0, 5, 5], [("fused", 512, True, 1)], min_grad=[0.0, 1e-9, 1e-9]),
    "split_320x240": _form((320, 240), [0, 5, 5], [("persistent", 512, True, 2), ("persistent", 512, True, 1)],
                           min_grad=[0.0, 1e-9, 1e-9], fusion=native.FUSION_SPLIT),
    "slide_320x240": _form((320, 240), [4], [("slide", 768, False, 0), ("slide_fallback", 1024, False, 0)], slide_policy=0),
    "exact_320x240": _form((320, 240), [4], [("persistent", 1024, False, 0)], slide_policy=-1),
    "fallback_320x240": _form((320, 240), [6], [("slide", 768, False, 0), ("slide_fallback", 1024, False, 0)],
                              slide_policy=0, leaves_window=True),
    # 655 360 pixels: the in-bounds ballots of a pair (80 KB) no longer fit beside the kernel's LDS: global memory
    "ballots_hbm_1024x640": _form((1024, 640), [2], [("persistent", 1024, False, 0)], slide_policy=-1, storages=[native.STORAGE_F16]),
}
LATENCY_BATCH = 8                # the latency forms are what batches of <= 8 pairs take: that is their largest batch


def form_cells():
    """(form, storage, huber on) of part 1."""
    out = []
    for name, f in FORMS.items():
        for st in f["settings"].get("storages", STORAGES):
            for hub in (False, True):
                out.append((name, st, hub))
    return out


def cell_id(cell):
    name, st, hub = cell
    return f"{name}-{STORAGE_IDS[st]}-{'huber' if hub else 'plain'}"


def configs(max_iter, min_grad=None, **depth):
    nl = len(max_iter)
    mg = [0.0] * nl if min_grad is None else min_grad
    return (native.make_config(num_levels=nl, max_iter=max_iter, min_grad=mg),
            oracle.make_config(num_levels=nl, max_iter=max_iter, min_grad=mg, **depth))


def huber_deltas(max_iter, on):
    return [DELTA if m > 0 else 0.0 for m in max_iter] if on else None


def occlude(p):
    """An occluder-like block of 255 in the target: residuals of ~0.5 there, ten times DELTA."""
    h, w = p["gray1"].shape
    g1 = p["gray1"].copy()
    g1[h // 4:h // 4 + max(h // 6, 1), w // 3:w // 3 + max(w // 5, 1)] = 255
    q = dict(p)
    q["gray1"] = g1
    return q


def form_pairs(name):
    """A handful of distinct pairs of a form: [(pair, initial state)], the first one the pair that gets the subnormal
    patches."""
    f = FORMS[name]
    w, h = f["size"]
    if f["settings"].get("leaves_window"):
        # an in-plane rotation of 0.3 rad moves the border pixels by ~48 rows at 320x240, more than the window covers
        # (test_sliding_window_hands_large_motions_to_the_exact_kernel): out at once, drifting out, and two that stay
        big = synthetic.render_pair_with_motion(91, w, h, [0.01, -0.005, 0.004, 0.30, 0.002, -0.003])
        small = [synthetic.make_pair(92 + i, w, h, holes=0.02, trans=0.01, rot=0.004) for i in range(2)]
        near = big["motion"] + np.array([0.004, 0.002, -0.003, 0.004, -0.002, 0.001])
        drift = np.array([0.0, 0.0, 0.0, 0.17, 0.0, 0.0])
        return [(occlude(small[0]), np.zeros(6)), (occlude(big), near), (occlude(big), drift), (occlude(small[1]), np.zeros(6))]
    n = 3 if w * h > 400000 else 4
    rs = np.random.RandomState(w * 1000 + h)
    out = []
    for i in range(n):
        p = synthetic.make_pair(200 + i, w, h, holes=0.02, trans=0.008 * (i + 1), rot=0.003 * (i + 1))
        init = np.zeros(6) if i % 2 == 0 else rs.uniform(-1, 1, 6) * np.array([0.01, 0.01, 0.01, 0.004, 0.004, 0.004])
        out.append((occlude(p), init))
    return out


def batch_order(n_distinct, n=N_BATCH, seed=9):
    """A shuffled batch in which every distinct pair occurs."""
    order = np.random.RandomState(seed).randint(0, n_distinct, size=n)
    order[:n_distinct] = np.arange(n_distinct)
    return [int(i) for i in order]


# ------------------------------------------------------------------------------------------------------------------------
# fp16 subnormals: a dark patch (source and target intensity) and a flat patch (target gradients)
# ------------------------------------------------------------------------------------------------------------------------
def _dark(h, w):
    return slice(h // 2, h // 2 + max(h // 5, 1)), slice(w // 8, w // 8 + max(w // 4, 1))


def _flat(h, w):
    return slice(h // 4, h // 4 + max(h // 6, 1) + max(h // 8, 1)), slice(w // 3, w // 3 + max(w // 5, 1) + max(w // 8, 1))


def subnormal_patches(i0, i1, gx, gy):
    """Copies of a level's planes with the dark patch's intensities (in [0, 1]) and the flat patch's gradients (|g| <= 1)
    scaled by 6e-5, i.e. into fp16's subnormal range (< 6.1e-5).  The gradients over the dark patch and the residuals
    over the flat one keep their size, so a load that flushed subnormals to zero would move the normal equations by ~1e-5
    relative -- four orders above the pose bar."""
    h, w = i1.shape
    i0, i1, gx, gy = i0.copy(), i1.copy(), gx.copy(), gy.copy()
    i0[_dark(h, w)] *= 6e-5
    i1[_dark(h, w)] *= 6e-5
    gx[_flat(h, w)] *= 6e-5
    gy[_flat(h, w)] *= 6e-5
    return i0, i1, gx, gy


def count_f16_subnormals(a):
    a = np.abs(a[np.isfinite(a)])
    return int(np.sum((a > 0) & (a < F16_MIN_NORMAL)))


def emulated_planes(ocfg, p, storage, patched=False):
    """The five plane lists the device would hold for pair p under `storage`: the oracle's fp64 pyramids rounded once;
    patched: subnormal_patches applied to the rounded planes of every active level and rounded again, as get_level_planes
    -> set_level_planes does."""
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    out = [[], [], [], [], []]
    for l in range(ocfg.num_levels):
        if ocfg.max_num_iterations[l] > 0:
            i0, i1, gx, gy = [round_image(a[l], storage) for a in (i0p, i1p, gxp, gyp)]
            d0 = round_depth(d0p[l], storage)
            if patched:
                i0, i1, gx, gy = [round_image(a, storage) for a in subnormal_patches(i0, i1, gx, gy)]
        else:
            i0 = d0 = i1 = gx = gy = np.zeros_like(i0p[l])
        for lst, v in zip(out, (i0, d0, i1, gx, gy)):
            lst.append(v)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# expectations
# ------------------------------------------------------------------------------------------------------------------------
def expect(ocfg, K, planes, init, huber=None, **ext):
    """Expect (the oracle's result, the conditioned bar 1e-9 x max(1, cond / 1e5) capped at 1e-5, the one-ulp-of-fx
    guard) on the given planes."""
    return Expect(ocfg, K, planes, init, huber_delta=huber, **ext)


def huber_bites(ocfg, K, planes, init, huber):
    """Fraction of the coarsest active level's residuals at the initial state that lie beyond that level's delta, i.e.
    whose Huber weight is below 1.  (Nearest-neighbour residuals; the occluder block is wide enough that the bilinear ones
    exceed delta on it as well.)"""
    l = max(l for l in range(ocfg.num_levels) if ocfg.max_num_iterations[l] > 0)
    i0p, d0p, i1p, gxp, gyp = planes
    r, _ = oracle.compute_residuals_and_jacobians(i0p[l], d0p[l], i1p[l], gxp[l], gyp[l], l, K, init,
                                                  ocfg.min_depth, ocfg.max_depth)
    r = r[np.isfinite(r)]
    return float(np.mean(np.abs(r) > huber[l])) if r.size else 0.0


def ratio(state, e):
    """distance / bar of a device state against an Expect (0 where the oracle itself is not finite)."""
    return se3.state_distance(state, e.state) / e.bar if e.finite else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# part 2: bilinear
# ------------------------------------------------------------------------------------------------------------------------
# 75x53 = 3975 pixels: not a multiple of the workgroup's stride (256); 9x7 = 63 pixels: one partial chunk; 160x120
BILINEAR_SIZES = [((75, 53), [4]), ((9, 7), [2]), ((160, 120), [4])]
BILINEAR_STORAGES = [native.STORAGE_F16, native.STORAGE_F64, native.STORAGE_F32]       # record form; DMA form x 2


def bilinear_cells():
    return [(st, c, hub) for st in BILINEAR_STORAGES for c in (False, True) for hub in (False, True)]


def bilinear_id(cell):
    st, c, hub = cell
    return f"{STORAGE_IDS[st]}-{'corrected' if c else 'reference'}-{'huber' if hub else 'plain'}"


def bilinear_pairs(size):
    w, h = size
    if w * h < 64:
        # Rendered larger and cropped, the principal point moved with the crop; a 2 x 2 occluder.  63 pixels hold six
        # parameters loosely: small motions and two iterations are what the one-ulp guard accepts (three iterations, or
        # other seeds, run away on the oracle itself).
        out = []
        for i in range(3):
            p = synthetic.make_pair(300 + i, 64, 48, holes=0.0, trans=0.002 * (i + 1), rot=0.001 * (i + 1))
            q = {k: np.ascontiguousarray(p[k][20:20 + h, 28:28 + w]) for k in ("gray0", "depth0", "gray1", "depth1")}
            q["K"] = p["K"].copy()
            q["K"][0, 2] -= 28.0
            q["K"][1, 2] -= 20.0
            q["gray1"] = q["gray1"].copy()
            q["gray1"][1:3, 2:4] = 255
            out.append((q, np.zeros(6)))
        return out
    return [(occlude(synthetic.make_pair(300 + i, w, h, holes=0.02, trans=0.008 * (i + 1), rot=0.003 * (i + 1))), np.zeros(6))
            for i in range(3)]


# ------------------------------------------------------------------------------------------------------------------------
# part 3: edges
# ------------------------------------------------------------------------------------------------------------------------
GATE = (0.5, 4.0)                        # exact in fp32


def depth_gate_problem(w=80, h=60):
    """Level-0 planes of an 80x60 pair with depths planted that lie strictly inside GATE in fp64 and round to exactly its
    bounds in fp32 (a column near min_depth, a row near max_depth), plus NaN and negative depths.  -> K, planes (five
    one-level lists, fp64), number of planted pixels."""
    p = synthetic.make_pair(210, w, h, holes=0.0, trans=0.008, rot=0.003)
    _, ocfg = configs([1])
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    d0 = np.clip(d0p[0], 1.0, 3.0)                     # everything else well inside the gate
    lo, hi = GATE[0] * (1.0 + 1e-9), GATE[1] * (1.0 - 1e-9)
    assert GATE[0] < lo and hi < GATE[1] and np.float32(lo) == np.float32(GATE[0]) and np.float32(hi) == np.float32(GATE[1])
    planted = np.zeros((h, w), dtype=bool)
    planted[:, w // 3] = True
    d0[:, w // 3] = lo
    planted[h // 3, :] = True
    d0[h // 3, :] = hi
    d0[h // 2, ::3] = np.nan                           # not planted: excluded under every storage
    d0[h // 2 + 2, ::4] = -1.0
    planted &= np.isfinite(d0) & (d0 > 0)
    return p["K"], [[i0p[0]], [d0], [i1p[0]], [gxp[0]], [gyp[0]]], int(np.sum(planted))


def check_strip(e, ocfg, K, planes, init, huber, state, rep, what):
    """Expect.check where the oracle is finite.  Where it is not, a strip -- unlike the cases Expect was written for, which
    see no pixel from their first iteration on -- may lose its state after iterations that had valid pixels (a singular
    J^T J, or a step that throws every pixel out of the image).  The reference keeps iterating on the NaN and counts no
    pixel from then on; the device stops at the first non-finite state.  So the device is held to the
    oracle's trace up to exactly that iteration: its iteration counts and the valid pixels of its last iteration are the
    oracle's there, the pair is flagged PAIR_NONFINITE and its state is not finite."""
    if e.finite:
        e.check(state, rep, what)
        return
    nl = ocfg.num_levels
    _, _, tr = oracle.optimize(ocfg, K, *planes, init_state=init, want_trace=True, huber_delta=huber)
    its, valid = [0] * nl, [0] * nl
    for t in tr:
        its[t["level"]] += 1
        valid[t["level"]] = t["valid_pixels"]
        if not np.all(np.isfinite(t["state"])):
            break
    else:
        raise AssertionError((what, "the oracle's trace never loses its state"))
    assert list(rep.iterations[:nl]) == its, (what, list(rep.iterations[:nl]), its)
    assert list(rep.valid_pixels[:nl]) == valid, (what, list(rep.valid_pixels[:nl]), valid)
    assert rep.flags & native.PAIR_NONFINITE and not np.all(np.isfinite(state)), (what, rep.flags, state)


def strip_cases(w, h):
    """The strip of tests/test_gpu_objective_edges.py with the occluder block, and three initial states."""
    from test_gpu_objective_edges import _strip
    p = occlude(_strip(w, h))
    rs = np.random.RandomState(w * 1000 + h)
    return p, [np.zeros(6), p["motion"], rs.uniform(-0.02, 0.02, 6)]


def one_column_problem():
    """1 x 40 and 40 x 1 levels for bilinear sampling on fp64 planes: [(size, K, planes, target depth)].  The planes are a
    column / a row of a 64 x 48 pair's level 0 (so the gradients along the missing axis are not zero, and the oracle's normal
    equations have full rank: seed, motion and the two iterations are ones on which it stays finite and passes the guard).
    The target's depth plane has NaN holes where the 16-byte tap pair of a one-column row reaches: its first double (behind
    the intensity plane's last row) and the one below."""
    out = []
    p = synthetic.make_pair(34, 64, 48, holes=0.0, trans=0.006, rot=0.003)
    _, ocfg = configs([2])
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    for (w, h), (r0, c0) in (((1, 40), (4, 30)), ((40, 1), (20, 12))):
        planes = [[np.ascontiguousarray(a[0][r0:r0 + h, c0:c0 + w])] for a in (i0p, d0p, i1p, gxp, gyp)]
        K = p["K"].copy()
        K[0, 2] -= c0
        K[1, 2] -= r0
        depth1 = planes[1][0].copy()
        depth1.reshape(-1)[:2] = np.nan
        out.append(((w, h), K, planes, depth1))
    return out
