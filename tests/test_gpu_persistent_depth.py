"""Depth that stays parked in LDS across a level's iterations (csrc/gn_kernels.hip, level_body, PARK).

The first iteration a workgroup runs for a pair on a level loads every depth from memory and stores the leading
`depth_lds_chunks` chunks into the park block; every later iteration's pass 1 reads those chunks back from LDS and only
the others from memory.  Nothing about the arithmetic changes, so the bars are those of test_gpu_parity.py (identical
iteration counts, pose within 1e-9 of the oracle, gradient norm within 1e-9 relative) plus bit-identity wherever two runs
differ only in where a depth came from.

Shapes: the smallest that reach each case of the per-wave run selection (all chunks parked, the boundary inside a wave's
sequence, a partial last chunk on either side of it, both parities of the two-chunks-per-trip loop, fewer parked chunks
than waves).  The parked counts are recomputed from the planner's lds_bytes, not trusted.
"""
import functools

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9          # as tests/test_gpu_parity.py
WAVE = 64


def _cfgs(num_levels, max_iter, min_grad):
    kw = dict(num_levels=num_levels, blur=[0] * num_levels, grad_scale=[0.0625] * num_levels, lam=[1.0] * num_levels,
              max_iter=max_iter, min_grad=min_grad)
    return native.make_config(**kw), oracle.make_config(min_depth=0.3, max_depth=5.0, **kw)


def _parked_chunks(n, threads, lds_bytes):
    """Chunks the planner parks, from what it reports: LDS beyond the fixed block and the padded owner map, in 512-byte
    chunks (gn_plan_level: park_depth; lds_fixed_bytes; owner_lds_entries)."""
    fixed = 8 * (32 + 8 + (threads // WAVE) * 32) + 4 * 4
    owner = 4 * (((n + 63) & ~63) + threads)
    used = (fixed + owner + 7) & ~7
    left = lds_bytes - used
    assert left >= 0 and left % (8 * WAVE) == 0, (n, threads, lds_bytes)
    return left // (8 * WAVE)


def _parked_per_wave(chunks, parked, nw):
    return [len(range(w, parked, nw)) for w in range(min(nw, chunks))]


@functools.lru_cache(maxsize=None)
def _pair(w, h):
    return synthetic.make_pair(13, w, h, holes=0.03, trans=0.01 * w / 640, rot=0.004)


@functools.lru_cache(maxsize=None)
def _expected(w, h, iters):
    p = _pair(w, h)
    _, ocfg = _cfgs(1, [iters], [0.0])
    return oracle.align_frames(ocfg, p["K"], p["gray0"], p["depth0"], p["gray1"], want_trace=True)


# (width, height): threads, chunks, parked chunks (None: all of them)
SHAPES = {
    (32, 24): (64, 12, None),        # SOLO: one wave, every chunk parked
    (40, 30): (64, 19, 8),           # SOLO: the boundary inside the only wave's sequence; last chunk partial
    (60, 45): (256, 43, None),       # QUAD: the partial last chunk is parked
    (75, 53): (256, 63, 43),         # QUAD: the partial last chunk is not
    (80, 60): (256, 75, 37),         # QUAD: waves with 10 and 9 parked positions, both parities of the two-per-trip loop
    (128, 96): (512, 192, 55),       # MID
    (160, 120): (1024, 300, 153),    # WIDE: the headline launch
    (224, 168): (1024, 588, 9),      # WIDE: fewer parked chunks than waves, waves 9-15 have no parked run
}


def _check_geometry(size, info):
    w, h = size
    threads, chunks, parked = SHAPES[size]
    assert info["threads"] == threads and info["owner_in_lds"] and not info["source_in_lds"], info
    assert (w * h + WAVE - 1) // WAVE == chunks
    got = _parked_chunks(w * h, threads, info["lds_bytes"])
    assert got == (chunks if parked is None else parked), (size, got, info)
    per_wave = _parked_per_wave(chunks, got, threads // WAVE)
    if size == (40, 30):
        assert 0 < per_wave[0] < chunks and (w * h) % WAVE
    if size == (60, 45):
        assert (w * h) % WAVE and got == chunks
    if size == (75, 53):
        assert (w * h) % WAVE and got < chunks
    if size == (80, 60):
        assert sorted(set(per_wave)) == [9, 10]
    if size == (224, 168):
        assert got < threads // WAVE and per_wave.count(0) == threads // WAVE - got


@pytest.mark.parametrize("iters", [1, 2, 7])
@pytest.mark.parametrize("size", list(SHAPES), ids=[f"{w}x{h}" for w, h in SHAPES])
def test_each_shape_matches_the_oracle(size, iters):
    """One level, fixed iteration counts: 1 iteration is the first trip alone, 2 add exactly one trip that reads the park
    block, 7 several of them.  Nine copies of one pair: the throughput geometry, every copy the same bits."""
    w, h = size
    p = _pair(w, h)
    ncfg, _ = _cfgs(1, [iters], [0.0])
    es, eits, etr = _expected(w, h, iters)
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_intrinsic_matrix(p["K"])
        eng.reserve_frames(2, w, h)
        _check_geometry(size, eng.level_launch_info(0))
        eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
        eng.upload_frame(1, p["gray1"], None, roles=native.ROLE_TARGET)
        s, reps = eng.align_pairs([0] * 9, [1] * 9, want_reports=True)
        assert [r["kind"] for r in eng.last_launches()] == ["persistent"]
    assert eits == [iters]
    g_last = np.linalg.norm(etr[-1]["gradient"])
    for i in range(9):
        assert list(reps[i].iterations[:1]) == eits
        assert reps[i].flags == 0
        assert abs(reps[i].gradient_norm - g_last) <= 1e-9 * max(1.0, g_last)
        assert np.array_equal(s[i], s[0])
    d = se3.state_distance(s[0], es)
    print(f"{w}x{h}, {iters} iterations: pose distance {d:.3e}")
    assert d < POSE_TOL


@pytest.mark.parametrize("storage", [native.STORAGE_F32, native.STORAGE_F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("size", [(80, 60), (160, 120)], ids=["80x60", "160x120"])
def test_narrow_storage_matches_the_extended_oracle(size, storage):
    """The park block holds the converted double whatever the planes are stored as: fp32 planes and fp16 images + fp32 depth
    against the oracle run on exactly the planes the device holds (as tests/test_gpu_extensions.py does)."""
    w, h = size
    p = _pair(w, h)
    ncfg, ocfg = _cfgs(1, [7], [0.0])
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_extensions(native.make_extensions(plane_storage=storage))
        eng.set_intrinsic_matrix(p["K"])
        eng.reserve_frames(2, w, h)
        info = eng.level_launch_info(0)
        assert info["owner_in_lds"] and not info["source_in_lds"], info
        parked = _parked_chunks(w * h, info["threads"], info["lds_bytes"])
        assert 0 < parked < (w * h + WAVE - 1) // WAVE, (info, parked)         # some chunks from LDS, some from memory
        eng.upload_frame(0, p["gray0"], p["depth0"])
        eng.upload_frame(1, p["gray1"], p["depth1"])
        i0, d0, _, _ = eng.get_level_planes(0, 0)
        i1, _, gx, gy = eng.get_level_planes(1, 0)
        es, eits, etr = oracle.optimize(ocfg, p["K"], [i0], [d0], [i1], [gx], [gy], want_trace=True)
        s, reps = eng.align_pairs([0] * 9, [1] * 9, want_reports=True)
    g_last = np.linalg.norm(etr[-1]["gradient"])
    for i in range(9):
        assert list(reps[i].iterations[:1]) == eits == [7]
        assert abs(reps[i].gradient_norm - g_last) <= 1e-9 * max(1.0, g_last)
        assert np.array_equal(s[i], s[0])
    assert se3.state_distance(s[0], es) < POSE_TOL


# ---------------------------------------------------------------------------------------------
# fused levels: 128x96 + 64x48 of a 512x384 pair
# ---------------------------------------------------------------------------------------------
FUSED_W, FUSED_H = 512, 384
FUSED_MIN_GRAD = [0.0, 0.0, 100.0, 60.0]     # gradient norms of these pairs run from ~1000 down to ~20 on the two levels


def _report_tuple(r, nl):
    return (list(r.iterations[:nl]), list(r.valid_pixels[:nl]), r.gradient_norm, r.flags)


def _upload(eng, probs):
    eng.reserve_frames(2 * len(probs), probs[0]["gray0"].shape[1], probs[0]["gray0"].shape[0])
    for i, p in enumerate(probs):
        eng.upload_frame(2 * i, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
        eng.upload_frame(2 * i + 1, p["gray1"], None, roles=native.ROLE_TARGET)


def test_parked_equals_unparked_bit_for_bit_in_the_fused_geometry():
    """Levels 128x96 and 64x48 as one fused launch, as the same 512-thread geometry launched level by level, and in each
    level's own geometry.  The fused launch parks ALL of 64x48 in the owner map's unused tail and none of 128x96; the
    level-by-level launches of that geometry park nothing -- the same arithmetic with every depth from memory in every
    iteration -- so the two must agree bit for bit.  With one launch per level in its own geometry 128x96 is a MID launch
    that parks 55 of 192 chunks: the oracle's result within the bar.  Five pairs of different motions, so that pairs leave
    the levels after different iteration counts."""
    nl, max_iter = 4, [0, 0, 6, 9]
    ncfg, ocfg = _cfgs(nl, max_iter, FUSED_MIN_GRAD)
    probs = [synthetic.make_pair(50 + i, FUSED_W, FUSED_H, holes=0.02, trans=0.006 * (i + 1), rot=0.003 * (i + 1))
             for i in range(5)]
    expect = [oracle.align_frames(ocfg, p["K"], p["gray0"], p["depth0"], p["gray1"]) for p in probs]
    assert len({tuple(e[1]) for e in expect}) > 1, [e[1] for e in expect]
    assert any(1 < e[1][3] for e in expect) and any(1 < e[1][2] for e in expect)       # trips that read the park block
    src, tgt = [0, 2, 4, 6, 8], [1, 3, 5, 7, 9]
    out, launches = {}, {}
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_intrinsic_matrix(probs[0]["K"])
        _upload(eng, probs)
        for mode in (native.FUSION_AUTO, native.FUSION_SPLIT, native.FUSION_OFF):
            eng.set_level_fusion(mode)
            out[mode] = eng.align_pairs(src, tgt, want_reports=True)
            launches[mode] = eng.last_launches()
    auto, split, off = (launches[m] for m in (native.FUSION_AUTO, native.FUSION_SPLIT, native.FUSION_OFF))
    assert [(r["kind"], r["levels"], r["threads"]) for r in auto] == [("fused", [3, 2], 512)], auto
    assert [(r["kind"], r["levels"], r["threads"]) for r in split] == [("persistent", [3], 512), ("persistent", [2], 512)], split
    # the fused launch's LDS is sized for 128x96 alone: 64x48 (48 chunks) fits the tail that level leaves, 128x96 has none
    n2, n3 = 128 * 96, 64 * 48
    assert _parked_chunks(n2, 512, auto[0]["lds_bytes"]) == 0
    assert (n2 - n3) * 4 // (8 * WAVE) >= n3 // WAVE
    assert all(r["lds_bytes"] <= auto[0]["lds_bytes"] for r in split), split                 # no room beyond the maps: nothing parked
    assert [r["kind"] for r in off] == ["persistent", "persistent"] and off[1]["levels"] == [2] and off[1]["threads"] == 512
    assert _parked_chunks(n2, 512, off[1]["lds_bytes"]) == 55
    a, s = out[native.FUSION_AUTO], out[native.FUSION_SPLIT]
    assert np.array_equal(a[0], s[0])
    assert [_report_tuple(r, nl) for r in a[1]] == [_report_tuple(r, nl) for r in s[1]]
    for mode, (st, reps) in out.items():
        for i, (es, eits) in enumerate(expect):
            assert list(reps[i].iterations[:nl]) == eits, (mode, i, list(reps[i].iterations[:nl]), eits)
            assert se3.state_distance(st[i], es) < POSE_TOL, (mode, i)
            assert reps[i].flags == 0


# ---------------------------------------------------------------------------------------------
# a workgroup's park block never serves another pair
# ---------------------------------------------------------------------------------------------
def _two_scenes(w, h):
    return [synthetic.make_pair(71, w, h, holes=0.03, trans=0.01 * w / 640, rot=0.004, scene="plane"),
            synthetic.make_pair(902, w, h, trans=0.02 * w / 640, rot=0.006, scene="layered")]


@pytest.mark.parametrize("size,threads,n_pairs", [((160, 120), 1024, 260), ((80, 60), 256, 1030), ((FUSED_W, FUSED_H), 512, 520)],
                         ids=["wide", "quad", "fused"])
def test_no_stale_depth_between_pairs(size, threads, n_pairs):
    """More pairs than the persistent grid has workgroups (256 x 1, 256 x 4, 256 x 2), alternating between two very
    different scenes: every workgroup draws several pairs in succession, and the park block it filled for one must not
    serve the next.  Every pair equals, bit for bit, the same pair aligned alone."""
    w, h = size
    fused = threads == 512
    if fused:
        nl = 4
        ncfg, _ = _cfgs(nl, [0, 0, 3, 3], [0.0, 0.0, 1e-3, 1e-3])     # a threshold, so that the levels fuse; nobody meets it
    else:
        nl = 1
        ncfg, _ = _cfgs(nl, [3], [0.0])
    probs = _two_scenes(w, h)
    assert not np.array_equal(probs[0]["depth0"], probs[1]["depth0"])
    src = [2 * (k % 2) for k in range(n_pairs)]
    tgt = [2 * (k % 2) + 1 for k in range(n_pairs)]
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_intrinsic_matrix(probs[0]["K"])
        _upload(eng, probs)
        alone = []
        for i in range(2):
            st, rp = eng.align_pairs([2 * i], [2 * i + 1], want_reports=True)
            alone.append((st[0].copy(), _report_tuple(rp[0], nl)))
            one = eng.last_launches()
        states, reps = eng.align_pairs(src, tgt, want_reports=True)
        many = eng.last_launches()
    assert [(r["kind"], r["threads"]) for r in many] == [("fused" if fused else "persistent", threads)], many
    assert [(r["kind"], r["threads"], r["lds_bytes"]) for r in one] == [(r["kind"], r["threads"], r["lds_bytes"]) for r in many]
    assert many[0]["workgroups"] < n_pairs, many
    if fused:
        assert alone[0][1][0][2:] == [3, 3] and alone[1][1][0][2:] == [3, 3], alone
    assert not np.array_equal(alone[0][0], alone[1][0])
    for k in range(n_pairs):
        assert np.array_equal(states[k], alone[k % 2][0]), k
        assert _report_tuple(reps[k], nl) == alone[k % 2][1], k
