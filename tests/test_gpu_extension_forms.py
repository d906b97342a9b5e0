"""The opt-in extensions of the photometric objective -- fp32 / fp16 plane storage, Huber weights, bilinear sampling with or
without the corrected Jacobian -- on every launch form, against the oracle extended identically and fed the planes exactly
as the device stored them (run with -m gpu on an MI355X).  Inputs: tests/extension_forms.py, vouched for on the CPU by
tests/test_extensions_cpu.py (finite, well-posed, Huber weights below 1).

1. form x storage x Huber on the scatter path: the 64- / 256- / 512- / 1024-thread geometries of gn_level_kernel, the
   latency forms, the fused launch and the same geometry split, the sliding-window kernel, the exact kernel with the owner
   map in HBM, pairs that leave the window and are finished by the exact kernel, and a level whose in-bounds ballots live in
   HBM.  One pair, then 640 shuffled copies of a handful of pairs (one work queue per XCD): the oracle's iteration counts,
   valid pixels and flags, the pose within 1e-9 x max(1, cond(J^T J) / 1e5) (capped at 1e-5), every copy the same bits, on
   levels whose owner map is in LDS the same bits as the pair aligned alone, fused and split the same bits.  (The latency
   forms are what batches of <= 8 pairs take: 8 is their batch.)  The first pair of every cell carries fp16-subnormal
   intensities and gradients, so a load conversion that flushed them would miss the bar in that form.
2. the bilinear kernels (fp16 record form, fp64 / fp32 LDS-DMA form) x corrected x Huber at 75x53, 9x7 and 160x120.
3. edges of the narrow storages: the depth gate after rounding, fp16 subnormals and overflow, narrow strips, one-column and
   one-row levels under bilinear sampling with NaN in the target's depth plane.
4. `sampling` toggled on resident fp16 frames: the pool is dropped, the next align is refused with PHOVO_E_NOT_READY.
5. tests/tools/fuzz_parity.py in its `ext` and `ext big` modes.
Every test asserts from last_launches() that the form it names ran and prints the largest distance / bar it met.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import extension_forms as ef
from test_gpu_objective_edges import _assert_geometry

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "fuzz_parity.py")


def _assert_launches(launches, expected, sizes):
    """Every launch of an enqueue, one by one through _assert_geometry: (kind, threads, owner map in LDS, level)."""
    assert len(launches) == len(expected), launches
    for rec, (kind, threads, in_lds, level) in zip(launches, expected):
        w, h = sizes[level]
        _assert_geometry([rec], kind, threads, in_lds, w * h)


def _engine(ncfg, K, storage, huber, size, n_frames, sampling=native.SAMPLING_NEAREST_SCATTER, corrected=False, **settings):
    e = odometry.AlignmentEngine()
    e.set_config(ncfg)
    e.set_extensions(native.make_extensions(plane_storage=storage, huber_delta=huber, sampling=sampling,
                                            jacobian_corrected=corrected))
    e.set_intrinsic_matrix(K)
    e.set_wide_policy(-1)                      # one pair takes the form the test names, not the many-workgroups form
    if "slide_policy" in settings:
        e.set_slide_policy(settings["slide_policy"])
    if "fusion" in settings:
        e.set_level_fusion(settings["fusion"])
    if settings.get("latency"):
        e.set_latency_forms(True)
    e.reserve_frames(n_frames, size[0], size[1])
    return e


def _stored(eng, src, tgt, max_iter, size):
    """Oracle inputs = exactly the planes the device holds for the pair (src, tgt); levels it does not hold: zeros."""
    planes = [[], [], [], [], []]
    for l in range(len(max_iter)):
        if max_iter[l] > 0:
            i0, d0, _, _ = eng.get_level_planes(src, l)
            i1, _, gx, gy = eng.get_level_planes(tgt, l)
        else:
            lw, lh = oracle.level_size(size[0], size[1], l)
            i0 = d0 = i1 = gx = gy = np.zeros((lh, lw))
        for lst, v in zip(planes, (i0, d0, i1, gx, gy)):
            lst.append(v)
    return planes


def _upload_pairs(eng, pairs):
    for k, (p, _) in enumerate(pairs):
        eng.upload_frame(2 * k, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
        eng.upload_frame(2 * k + 1, p["gray1"], None, roles=native.ROLE_TARGET)


def _plant_subnormals(eng, src, tgt, max_iter, storage):
    """extension_forms.subnormal_patches on every active level of one pair, through get_level_planes / set_level_planes; the
    stored planes are numpy's rounding of what was set, bit for bit (nothing flushed to zero)."""
    for l in range(len(max_iter)):
        if max_iter[l] <= 0:
            continue
        i0, d0, _, _ = eng.get_level_planes(src, l)
        i1, _, gx, gy = eng.get_level_planes(tgt, l)
        i0, i1, gx, gy = ef.subnormal_patches(i0, i1, gx, gy)
        eng.set_level_planes(src, l, intensity=i0, depth=d0)
        eng.set_level_planes(tgt, l, intensity=i1, grad_x=gx, grad_y=gy)
        s0, sd, _, _ = eng.get_level_planes(src, l)
        s1, _, sx, sy = eng.get_level_planes(tgt, l)
        for got, want in ((s0, i0), (s1, i1), (sx, gx), (sy, gy)):
            assert np.array_equal(got, ef.round_image(want, storage)), l
            if storage == native.STORAGE_F16:
                assert ef.count_f16_subnormals(got) >= 8, l
        assert np.array_equal(sd, d0, equal_nan=True), l


def _batch(pairs, n):
    order = ef.batch_order(len(pairs), n)
    return order, [2 * i for i in order], [2 * i + 1 for i in order], np.stack([pairs[i][1] for i in order])


# ------------------------------------------------------------------------------------------------------------------------
# 1. form x storage x Huber on the scatter path
# ------------------------------------------------------------------------------------------------------------------------
def _run_form(name, storage, hub):
    """Align the form's pairs one at a time and in a shuffled batch.  -> dict(single, batch, reports, order, expects,
    worst)."""
    f = ef.FORMS[name]
    size, max_iter, settings = f["size"], f["max_iter"], f["settings"]
    nl = len(max_iter)
    sizes = [oracle.level_size(size[0], size[1], l) for l in range(nl)]
    ncfg, ocfg = ef.configs(max_iter, f["min_grad"])
    huber = ef.huber_deltas(max_iter, hub)
    pairs = ef.form_pairs(name)
    n_batch = ef.LATENCY_BATCH if settings.get("latency") else ef.N_BATCH
    with _engine(ncfg, pairs[0][0]["K"], storage, huber, size, 2 * len(pairs), **settings) as eng:
        _upload_pairs(eng, pairs)
        _plant_subnormals(eng, 0, 1, max_iter, storage)
        planes = [_stored(eng, 2 * k, 2 * k + 1, max_iter, size) for k in range(len(pairs))]
        single = []
        for k, (_, init) in enumerate(pairs):
            single.append(eng.align_pairs([2 * k], [2 * k + 1], init_states=init[None], want_reports=True))
            _assert_launches(eng.last_launches(), f["launches"], sizes)
        order, src, tgt, inits = _batch(pairs, n_batch)
        states, reps = eng.align_pairs(src, tgt, init_states=inits, want_reports=True)
        _assert_launches(eng.last_launches(), f["launches"], sizes)
        in_lds = all(rec[2] for rec in f["launches"])
    expects = [ef.expect(ocfg, p["K"], planes[k], init, huber) for k, (p, init) in enumerate(pairs)]
    worst = 0.0
    first = {i: order.index(i) for i in range(len(pairs))}
    for k, e in enumerate(expects):
        assert e.finite, (name, k)
        s1, r1 = single[k]
        e.check(s1[0], r1[0], (name, "one pair", k))
        e.check(states[first[k]], reps[first[k]], (name, "batch", k))
        worst = max(worst, ef.ratio(s1[0], e), ef.ratio(states[first[k]], e))
        if in_lds:                                   # a pair's bits do not depend on its batch
            assert np.array_equal(s1[0], states[first[k]]), (name, k)
    for pos, i in enumerate(order):                  # every copy of a pair: the same bits, whatever its workgroup did before
        assert np.array_equal(states[pos], states[first[i]]), (name, pos, i)
        a, b = reps[pos], reps[first[i]]
        assert list(a.iterations[:nl]) == list(b.iterations[:nl]) and list(a.valid_pixels[:nl]) == list(b.valid_pixels[:nl])
        assert a.flags == b.flags and a.gradient_norm == b.gradient_norm, (name, pos, i)
    if hub:                                          # the weights changed the estimate
        for k, (p, init) in enumerate(pairs):
            plain = ef.expect(ocfg, p["K"], planes[k], init, None)
            assert se3.state_distance(expects[k].state, plain.state) > 1e-6, (name, k)
            assert se3.state_distance(single[k][0][0], plain.state) > 1e-6, (name, k)
    return dict(single=single, batch=states, reports=reps, order=order, first=first, expects=expects, worst=worst)


SCATTER_CELLS = [c for c in ef.form_cells() if not c[0].startswith(("fused", "split"))]


@pytest.mark.parametrize("cell", SCATTER_CELLS, ids=[ef.cell_id(c) for c in SCATTER_CELLS])
def test_scatter_form_with_narrow_storage_and_huber(cell):
    name, storage, hub = cell
    out = _run_form(name, storage, hub)
    f = ef.FORMS[name]
    if f["settings"].get("leaves_window"):
        # pair 1 (0.3 rad in plane from its first iteration) left the sliding window and was finished by the exact kernel's
        # narrow / Huber instantiation; pair 2 starts at 0.17 rad and may follow it; pairs 0 and 3 stayed
        allowed = {0: (0,), 1: (native.PAIR_WINDOW_FALLBACK,), 2: (0, native.PAIR_WINDOW_FALLBACK), 3: (0,)}
        for pos, i in enumerate(out["order"]):
            assert out["reports"][pos].flags in allowed[i], (pos, i, out["reports"][pos].flags)
        for k in range(4):
            assert out["single"][k][1][0].flags in allowed[k], k
    else:
        assert all(r.flags == 0 for r in out["reports"])
    print(f"{ef.cell_id(cell)}: launches {f['launches']}, worst distance / bar {out['worst']:.3f}")


FUSED_CELLS = [(st, hub) for st in ef.STORAGES for hub in (False, True)]


@pytest.mark.parametrize("storage,hub", FUSED_CELLS, ids=[f"{ef.STORAGE_IDS[s]}-{'huber' if h else 'plain'}" for s, h in FUSED_CELLS])
def test_fused_and_split_launches_with_narrow_storage_and_huber(storage, hub):
    """Levels 2 and 1 of a 320x240 pyramid (80x60, 160x120) as one fused launch and as the same geometry level by level:
    each against the oracle, and bit for bit against each other (states, gradient norms, valid pixels)."""
    fused = _run_form("fused_320x240", storage, hub)
    split = _run_form("split_320x240", storage, hub)
    assert np.array_equal(fused["batch"], split["batch"])
    for k in range(len(fused["single"])):
        assert np.array_equal(fused["single"][k][0], split["single"][k][0]), k
    for a, b in zip(fused["reports"], split["reports"]):
        assert a.gradient_norm == b.gradient_norm and list(a.valid_pixels[:3]) == list(b.valid_pixels[:3]) and a.flags == b.flags == 0
    print(f"fused / split {ef.STORAGE_IDS[storage]} huber {hub}: launches {ef.FORMS['fused_320x240']['launches']} / "
          f"{ef.FORMS['split_320x240']['launches']}, worst distance / bar {max(fused['worst'], split['worst']):.3f}")


# ------------------------------------------------------------------------------------------------------------------------
# 2. bilinear kernels
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ef.bilinear_cells(), ids=[ef.bilinear_id(c) for c in ef.bilinear_cells()])
def test_bilinear_kernels_at_odd_tiny_and_full_sizes(cell):
    """The fp16 record form and the fp64 / fp32 LDS-DMA form, with and without the corrected Jacobian and Huber weights, at
    75x53 (3975 pixels: not a multiple of the workgroup's 256), 9x7 (63 pixels: one partial chunk) and 160x120; one pair
    and 640 shuffled copies of three pairs."""
    storage, corrected, hub = cell
    worst = 0.0
    for size, max_iter in ef.BILINEAR_SIZES:
        ncfg, ocfg = ef.configs(max_iter)
        huber = ef.huber_deltas(max_iter, hub)
        pairs = ef.bilinear_pairs(size)
        ext = dict(bilinear=True, corrected=corrected)
        with _engine(ncfg, pairs[0][0]["K"], storage, huber, size, 2 * len(pairs), sampling=native.SAMPLING_BILINEAR,
                     corrected=corrected) as eng:
            _upload_pairs(eng, pairs)
            planes = [_stored(eng, 2 * k, 2 * k + 1, max_iter, size) for k in range(len(pairs))]
            single = []
            for k in range(len(pairs)):
                single.append(eng.align_pairs([2 * k], [2 * k + 1], want_reports=True))
                _assert_geometry(eng.last_launches(), "bilinear", 256, False, size[0] * size[1])
            order, src, tgt, inits = _batch(pairs, ef.N_BATCH)
            states, reps = eng.align_pairs(src, tgt, init_states=inits, want_reports=True)
            _assert_geometry(eng.last_launches(), "bilinear", 256, False, size[0] * size[1])
        first = {i: order.index(i) for i in range(len(pairs))}
        for k, (p, init) in enumerate(pairs):
            e = ef.expect(ocfg, p["K"], planes[k], init, huber, **ext)
            assert e.finite, (size, k)
            e.check(single[k][0][0], single[k][1][0], (size, "one pair", k))
            e.check(states[first[k]], reps[first[k]], (size, "batch", k))
            assert np.array_equal(single[k][0][0], states[first[k]]), (size, k)      # no owner map: one arithmetic per pair
            worst = max(worst, ef.ratio(single[k][0][0], e))
            if hub:
                plain = ef.expect(ocfg, p["K"], planes[k], init, None, **ext)
                assert se3.state_distance(single[k][0][0], plain.state) > 1e-6, (size, k)
        for pos, i in enumerate(order):
            assert np.array_equal(states[pos], states[first[i]]), (size, pos, i)
            assert reps[pos].flags == 0 and reps[pos].gradient_norm == reps[first[i]].gradient_norm
    print(f"bilinear {ef.bilinear_id(cell)}: 256 threads, sizes {[s for s, _ in ef.BILINEAR_SIZES]}, "
          f"worst distance / bar {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------
# 3. edges of the narrow storages
# ------------------------------------------------------------------------------------------------------------------------
def _set_planes(eng, src, tgt, planes, level=0, target_depth=None):
    i0p, d0p, i1p, gxp, gyp = planes
    eng.set_level_planes(src, level, intensity=i0p[level], depth=d0p[level])
    if target_depth is None:
        eng.set_level_planes(tgt, level, intensity=i1p[level], grad_x=gxp[level], grad_y=gyp[level])
    else:
        eng.set_level_planes(tgt, level, intensity=i1p[level], depth=target_depth, grad_x=gxp[level], grad_y=gyp[level])


def test_depth_gate_after_rounding_to_fp32():
    """min_depth 0.5 and max_depth 4.0 are exact in fp32.  Depths of 0.5 (1 + 1e-9) and 4.0 (1 - 1e-9) pass the (strict) gate
    in fp64 and sit exactly on it once stored as fp32: the narrow storages count exactly those pixels fewer than fp64
    storage, and each count is the oracle's on the stored planes.  NaN and negative depths in the same image."""
    K, planes, planted = ef.depth_gate_problem()
    h, w = planes[0][0].shape
    ncfg, ocfg = ef.configs([1], min_depth=ef.GATE[0], max_depth=ef.GATE[1])
    valid, worst = {}, 0.0
    for st in [native.STORAGE_F64] + ef.STORAGES:
        with _engine(ncfg, K, st, None, (w, h), 2) as eng:
            eng.set_depth_range(*ef.GATE)
            _set_planes(eng, 0, 1, planes)
            stored = _stored(eng, 0, 1, [1], (w, h))
            s, reps = eng.align_pairs([0] * 9, [1] * 9, want_reports=True)
            _assert_geometry(eng.last_launches(), "persistent", 256, True, w * h)
        assert np.array_equal(stored[1][0], ef.round_depth(planes[1][0], st), equal_nan=True)
        assert np.isnan(stored[1][0]).sum() > 0 and (stored[1][0] < 0).sum() > 0
        e = ef.expect(ocfg, K, stored, np.zeros(6))
        assert e.finite
        for k in range(9):
            e.check(s[k], reps[k], ("gate", st, k))
        worst = max(worst, ef.ratio(s[0], e))
        valid[st] = reps[0].valid_pixels[0]
    assert planted > 100
    for st in ef.STORAGES:
        assert valid[native.STORAGE_F64] - valid[st] == planted, (valid, planted)
    print(f"depth gate: persistent 256, valid pixels {valid}, planted {planted}, worst distance / bar {worst:.3f}")


def test_fp16_overflow_ends_its_pair_nonfinite_and_leaves_the_others_alone():
    """Intensities above 65504 given to set_level_planes under fp16 storage are stored as inf, as numpy rounds them; the
    pair that reads them ends PAIR_NONFINITE (the oracle's state on the stored planes is not finite either), a healthy pair
    in the same launch keeps its bits."""
    size, max_iter = (80, 60), [4]
    ncfg, ocfg = ef.configs(max_iter)
    pairs = ef.form_pairs("threads256_80x60")[:2]
    src, tgt = [0, 2] * 20, [1, 3] * 20
    with _engine(ncfg, pairs[0][0]["K"], native.STORAGE_F16, None, size, 4) as eng:
        _upload_pairs(eng, pairs)
        before, _ = eng.align_pairs(src, tgt, want_reports=True)
        i1, _, _, _ = eng.get_level_planes(3, 0)
        i1[20:30, 30:50] = 70000.0
        i1[31, 30] = 65520.0                       # the first value that rounds up to inf; 65519 below stays 65504
        i1[31, 31] = 65519.0
        eng.set_level_planes(3, 0, intensity=i1)
        got, _, _, _ = eng.get_level_planes(3, 0)
        assert np.array_equal(got, i1.astype(np.float32).astype(np.float16).astype(np.float64))
        assert np.isinf(got[20:30, 30:50]).all() and np.isinf(got[31, 30]) and got[31, 31] == 65504.0
        planes = _stored(eng, 2, 3, max_iter, size)
        after, reps = eng.align_pairs(src, tgt, want_reports=True)
        _assert_geometry(eng.last_launches(), "persistent", 256, True, size[0] * size[1])
    es, _ = oracle.optimize(ocfg, pairs[1][0]["K"], *planes)
    assert not np.all(np.isfinite(es))
    for k in range(40):
        if k % 2:
            assert reps[k].flags & native.PAIR_NONFINITE and not np.all(np.isfinite(after[k])), k
        else:
            assert reps[k].flags == 0 and np.array_equal(after[k], before[k]), k
    print("fp16 overflow: persistent 256, planted pair PAIR_NONFINITE, healthy pair bitwise unchanged")


def test_narrow_strips_on_the_scatter_path():
    """The strips of the objective-edge tests -- one to five pixels wide, and 75x53 -- on gn_level_kernel with each narrow
    storage, with and without Huber weights, from three initial states.  Such normal equations are often rank deficient:
    then both sides must lose their state at the same iteration, after the same valid pixels (extension_forms.check_strip);
    at most half of the 72 cases may be non-finite on the oracle."""
    cases = non_finite = 0
    worst = 0.0
    for w, h in ef.STRIPS:
        p, states = ef.strip_cases(w, h)
        ncfg, ocfg = ef.configs([3])
        for st in ef.STORAGES:
            for hub in (False, True):
                huber = ef.huber_deltas([3], hub)
                with _engine(ncfg, p["K"], st, huber, (w, h), 2) as eng:
                    _upload_pairs(eng, [(p, None)])
                    planes = _stored(eng, 0, 1, [3], (w, h))
                    s, reps = eng.align_pairs([0] * 3, [1] * 3, init_states=np.stack(states), want_reports=True)
                    _assert_geometry(eng.last_launches(), "persistent", 64 if w * h <= 2048 else 256, True, w * h)
                for k, init in enumerate(states):
                    e = ef.expect(ocfg, p["K"], planes, init, huber)
                    print(f"strip {(w, h)} {ef.STORAGE_IDS[st]} huber {hub} state {k}: device {s[k]} iterations "
                          f"{list(reps[k].iterations[:1])} valid {list(reps[k].valid_pixels[:1])} flags {reps[k].flags}; "
                          f"oracle {e.state} iterations {e.its} valid {e.valid}")
                    ef.check_strip(e, ocfg, p["K"], planes, init, huber, s[k], reps[k], (w, h, st, hub, k))
                    cases += 1
                    non_finite += not e.finite
                    worst = max(worst, ef.ratio(s[k], e))
    assert cases == 72 and 2 * non_finite <= cases, (non_finite, cases)
    print(f"strips: persistent 64 / 256, {non_finite} of {cases} cases non-finite on the oracle, "
          f"worst distance / bar {worst:.3f}")


def test_bilinear_on_one_column_and_one_row_levels_with_nan_in_the_target_depth():
    """W == 1 and H == 1 under bilinear sampling, the target's depth plane (a frame that serves as source and target) with
    NaN where a 16-byte tap pair at column 0 of a one-column row would reach: the first double behind the intensity plane's
    last row, and the one below.  The oracle never reads that depth and stays finite; the fp32 and fp16 forms (clamped taps,
    tap records) must too, in agreement with it, at both shapes, and the fp64 form on the one-row level.  The fp64 form on
    the one-column level is the one case phovo_hip.h excludes (finite target planes are its precondition there: the pair's
    second double is weighted by zero, not dropped): it runs on the finite depth plane and must agree with the oracle."""
    worst = 0.0
    for (w, h), K, planes, depth1 in ef.one_column_problem():
        ncfg, ocfg = ef.configs([2])
        e = ef.expect(ocfg, K, planes, np.zeros(6), None, bilinear=True, corrected=True)
        assert e.finite, (w, h)
        for st in (native.STORAGE_F64, native.STORAGE_F32, native.STORAGE_F16):
            with_nan = not (st == native.STORAGE_F64 and w < 2)
            with _engine(ncfg, K, st, None, (w, h), 2, sampling=native.SAMPLING_BILINEAR, corrected=True) as eng:
                _set_planes(eng, 0, 1, planes, target_depth=depth1 if with_nan else planes[1][0])
                _, d1, _, _ = eng.get_level_planes(1, 0)
                assert bool(np.isnan(d1.reshape(-1)[0]) and np.isnan(d1.reshape(-1)[1])) == with_nan
                stored = _stored(eng, 0, 1, [2], (w, h))
                s, reps = eng.align_pairs([0] * 3, [1] * 3, want_reports=True)
                _assert_geometry(eng.last_launches(), "bilinear", 256, False, w * h)
            es = e if st == native.STORAGE_F64 else ef.expect(ocfg, K, stored, np.zeros(6), None, bilinear=True, corrected=True)
            assert es.finite, (w, h, st)
            for k in range(3):
                assert np.all(np.isfinite(s[k])), (w, h, st, s[k])
                es.check(s[k], reps[k], (w, h, st, k))
                assert np.array_equal(s[k], s[0])
            worst = max(worst, ef.ratio(s[0], es))
    print(f"one-column / one-row bilinear: 256 threads, worst distance / bar {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------
# 4. state change
# ------------------------------------------------------------------------------------------------------------------------
def test_toggling_sampling_on_resident_fp16_frames_drops_the_pool():
    """phovo_hip.h, phovo_engine_set_extensions: fp16 planes carry tap records exactly under bilinear sampling, so changing
    `sampling` on them changes the pool's layout: the call returns PHOVO_OK, the frames are gone, the next align is refused
    with PHOVO_E_NOT_READY, and after reserve_frames + upload the engine aligns as a fresh one does.  On fp32 planes, and
    for a change of Huber deltas on fp16 ones, the frames stay."""
    size, max_iter = (80, 60), [4]
    ncfg, ocfg = ef.configs(max_iter)
    pairs = ef.form_pairs("threads256_80x60")[:1]
    p = pairs[0][0]
    nearest = native.make_extensions(plane_storage=native.STORAGE_F16)
    bilinear = native.make_extensions(plane_storage=native.STORAGE_F16, sampling=native.SAMPLING_BILINEAR)
    with _engine(ncfg, p["K"], native.STORAGE_F16, None, size, 2) as eng:
        _upload_pairs(eng, pairs)
        a = eng.align_pairs([0], [1])
        eng.set_extensions(native.make_extensions(plane_storage=native.STORAGE_F16, huber_delta=[ef.DELTA]))
        eng.align_pairs([0], [1])                                   # Huber deltas: the frames survive
        for ext, kind in ((bilinear, "bilinear"), (nearest, "persistent")):
            eng.set_extensions(ext)                                 # returns PHOVO_OK ...
            with pytest.raises(native.PhovoError) as err:           # ... and the frames are gone
                eng.align_pairs([0], [1])
            assert err.value.status == native.E_NOT_READY and "no frames resident" in str(err.value), str(err.value)
            eng.reserve_frames(2, *size)
            _upload_pairs(eng, pairs)
            planes = _stored(eng, 0, 1, max_iter, size)
            s, reps = eng.align_pairs([0], [1], want_reports=True)
            assert [r["kind"] for r in eng.last_launches()] == [kind]
            e = ef.expect(ocfg, p["K"], planes, np.zeros(6), None, bilinear=(kind == "bilinear"))
            e.check(s[0], reps[0], kind)
        assert np.array_equal(s, a)                                  # back on nearest sampling: the first result's bits
    with _engine(ncfg, p["K"], native.STORAGE_F32, None, size, 2) as eng:
        _upload_pairs(eng, pairs)
        eng.align_pairs([0], [1])
        eng.set_extensions(native.make_extensions(plane_storage=native.STORAGE_F32, sampling=native.SAMPLING_BILINEAR))
        eng.align_pairs([0], [1])                                   # fp32 planes carry no records: the frames survive
        assert [r["kind"] for r in eng.last_launches()] == ["bilinear"]
    print("sampling toggled on fp16 frames: pool dropped, PHOVO_E_NOT_READY at the next align; fp32 frames stay")


# ------------------------------------------------------------------------------------------------------------------------
# 5. the `ext` sweeps
# ------------------------------------------------------------------------------------------------------------------------
COMBINATIONS = [f"{st}/{sampling}/{hub}" for st in ("f64", "f32", "f16")
                for sampling in ("nearest", "bilinear", "bilinear-corrected") for hub in ("plain", "huber")]


@pytest.mark.parametrize("cases,seed,flags,kinds", [
    (80, 11, ("ext",), ("persistent", "fused", "slide", "slide_fallback", "wide", "bilinear")),
    (40, 11, ("ext", "big"), ("persistent", "bilinear", "slide", "slide_fallback")),
], ids=["ext", "ext_big"])
def test_randomised_sweep_of_the_extensions_against_oracle(cases, seed, flags, kinds):
    """tests/tools/fuzz_parity.py with `ext`: every case draws a storage, a sampling (nearest / bilinear / bilinear with the
    corrected Jacobian) and Huber weights or none; 0 failures, every one of the 18 combinations drawn at least once, every
    launch kind the mode can reach seen.  (Seeds chosen for that coverage, which is a property of the draws alone.)"""
    r = subprocess.run([sys.executable, TOOL, str(cases), str(seed), *flags], capture_output=True, text=True, timeout=900)
    out = r.stdout
    assert r.returncode == 0, out[-3000:] + r.stderr[-2000:]
    assert f"{cases} cases, 0 failures" in out, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith("extension combinations drawn")][0]
    for c in COMBINATIONS:
        m = re.search(rf"'{re.escape(c)}': (\d+)", line)
        assert m and int(m.group(1)) >= 1, (c, line)
    line = [l for l in out.splitlines() if l.startswith("launch kinds seen")][0]
    for k in kinds:
        m = re.search(rf"'{k}': (\d+)", line)
        assert m and int(m.group(1)) >= 1, (k, line)
    m = re.search(r"worst distance / bar ([0-9.]+)", out)
    assert m, out[-500:]
    print(f"{' '.join(flags)}: {line}; worst distance / bar {m.group(1)}")
