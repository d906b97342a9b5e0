"""GPU tests of the pyramid producers (csrc/pyramid_kernels.hip, through the C ABI) at the shapes that clip: widths of 1 to
3 pixels, levels that cross or end on the 256-thread block edge, clipped 2x2 blocks, clamped taps, blur kernels wider than
the image, batched uploads (blockIdx.z > 0), u16 depth and the bi-objective target planes on levels smaller than a workgroup.

Every stored plane is compared bit for bit with the CPU oracle AND held to the exact reference tests/pyramid_exact.py within
(roundings on the longest path) * 2^-53 * M -- the oracle and the kernels were written from one restatement, so only the
second comparison can see a mistake the two share (tests/test_pyramid_exact_cpu.py holds the oracle to the same reference).
Level sizes are checked against the exact rule.  Every test prints the worst ratio it met, in units of 2^-53 * M.
"""
from fractions import Fraction

import numpy as np
import pytest

import biobjective_ref as ref
import pyramid_exact as ex

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry
from oracle import oracle

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"{w}x{h}" for w, h in ex.SHAPES]
BLUR_IDS = [f"{w}x{h}-{'_'.join(map(str, b))}" for w, h, b in ex.BLUR_CASES]
K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1.0]])


def _cfgs(nl, blur=None, max_iter=None):
    kw = dict(num_levels=nl, blur=list(blur) if blur else [0] * nl, grad_scale=ex.GRAD_SCALES[:nl],
              max_iter=max_iter if max_iter else [1] * nl, min_grad=[0.0] * nl)
    return native.make_config(**kw), oracle.make_config(**kw)


def _engine(ncfg, frames, w, h, objective=None):
    e = odometry.AlignmentEngine(0)
    e.set_config(ncfg)
    if objective is not None:
        e.set_intrinsic_matrix(K)
        e.set_objective(objective)
    e.set_build_all_levels(True)
    e.reserve_frames(frames, w, h)
    return e


def _same_bits(a, b):
    """Bit for bit, NaN positions included (a NaN is a NaN whatever its sign and payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def _oracle_planes(gray, depth, ocfg):
    i1p, gxp, gyp = oracle.build_target_pyramids(gray, ocfg)
    _, d0p = oracle.build_source_pyramids(gray, depth, ocfg)
    return [(i1p[l], d0p[l], gxp[l], gyp[l]) for l in range(ocfg.num_levels)]


@pytest.mark.parametrize("w,h", ex.SHAPES, ids=SHAPE_IDS)
def test_planes_equal_oracle_and_exact(w, h):
    gray, depth = ex.frame(w, h)
    nl = ex.num_levels(w, h)
    ncfg, ocfg = _cfgs(nl)
    expect = _oracle_planes(gray, depth, ocfg)
    exact = ex.exact_levels(w, h)
    worst_resize = worst_scharr = 0.0
    with _engine(ncfg, 1, w, h) as e:
        e.upload_frame(0, gray, depth)
        for level in range(nl):
            assert e.level_size(level) == ex.level_size(w, h, level), level
            got = e.get_level_planes(0, level)
            for name, g, o in zip("I D GX GY".split(), got, expect[level]):
                assert _same_bits(g, o), (level, name)
            for g, (val, mag) in ((got[0], exact[level]["i"]), (got[1], exact[level]["d"])):
                r = ex.worst_ratio(g, val, mag)
                worst_resize = max(worst_resize, r)
                assert r <= ex.roundings_resize(level), (level, r)
            gx, mx, gy, my = ex.scharr(ex.to_plane(got[0]), ex.GRAD_SCALES[level])
            for g, val, mag in ((got[2], gx, mx), (got[3], gy, my)):
                r = ex.worst_ratio(g, val, mag)
                worst_scharr = max(worst_scharr, r)
                assert r <= ex.ROUNDINGS_SCHARR, (level, r)
    print(f"{w}x{h}, {nl} levels: resize worst {worst_resize:.3f} u*M (bound {ex.ROUNDINGS_RESIZE_1} / {ex.ROUNDINGS_RESIZE}), "
          f"Scharr worst {worst_scharr:.3f} u*M (bound {ex.ROUNDINGS_SCHARR})")


@pytest.mark.parametrize("w,h,resident0", [(75, 53, True), (77, 51, True), (75, 53, False)])
def test_blur_at_odd_shapes_equals_oracle(w, h, resident0):
    """Blur sizes [5, 3, 7, 0] on shapes whose levels clip, bit for bit; once more with level 0 not resident
    (max_num_iterations[0] = 0): the level-0 blur still feeds every later level."""
    gray, depth = ex.frame(w, h)
    blur = [5, 3, 7, 0]
    ncfg, ocfg = _cfgs(4, blur, max_iter=[1 if resident0 else 0, 1, 1, 1])
    expect = _oracle_planes(gray, depth, ocfg)
    with odometry.AlignmentEngine(0) as e:
        e.set_config(ncfg)
        e.reserve_frames(1, w, h)
        e.upload_frame(0, gray, depth)
        assert e.level_is_stored(0) == resident0
        for level in range(4):
            assert e.level_size(level) == ex.level_size(w, h, level)
            if not e.level_is_stored(level):
                continue
            for name, g, o in zip("I D GX GY".split(), e.get_level_planes(0, level), expect[level]):
                assert _same_bits(g, o), (level, name)


@pytest.mark.parametrize("w,h,blur", ex.BLUR_CASES, ids=BLUR_IDS)
def test_blur_wider_than_the_image_equals_oracle_and_exact(w, h, blur):
    gray, depth = ex.frame(w, h)
    nl = len(blur)
    assert nl == ex.num_levels(w, h)
    ncfg, ocfg = _cfgs(nl, blur)
    expect = _oracle_planes(gray, depth, ocfg)
    exact = ex.exact_blur_case(w, h, blur)
    worst = []
    with _engine(ncfg, 1, w, h) as e:
        e.upload_frame(0, gray, depth)
        for level in range(nl):
            got = e.get_level_planes(0, level)
            for name, g, o in zip("I D GX GY".split(), got, expect[level]):
                assert _same_bits(g, o), (level, name)
            val, mag, count = exact[level]
            r = ex.worst_ratio(got[0], val, mag)
            worst.append((round(r, 2), round(float(count), 1)))
            assert r <= count, (level, r, float(count))
            gx, mx, gy, my = ex.scharr(ex.to_plane(got[0]), ex.GRAD_SCALES[level])
            assert ex.worst_ratio(got[2], gx, mx) <= ex.ROUNDINGS_SCHARR and ex.worst_ratio(got[3], gy, my) <= ex.ROUNDINGS_SCHARR
    print(f"blur {w}x{h} {blur}: per level (worst u*M, bound) {worst}")


def test_loads_u8_and_u16():
    """convertTo(fp64, 1/255) of all 256 byte values, and double(u16) * scale at 0, 1, 65535 and a ramp."""
    gray = np.arange(256, dtype=np.uint8).reshape(16, 16)
    d16 = (np.arange(256, dtype=np.uint32) * 257).astype(np.uint16).reshape(16, 16)
    d16.flat[:3] = [0, 1, 65535]
    ncfg, _ = _cfgs(1)
    with _engine(ncfg, 2, 16, 16) as e:
        for f, scale in enumerate((1.0 / 5000.0, 1.0 / 1000.0)):
            e.upload_frame_u16(f, gray, d16, scale)
            i, d, _, _ = e.get_level_planes(f, 0)
            assert _same_bits(i, gray.astype(np.float64) * (1.0 / 255))
            assert _same_bits(d, d16.astype(np.float64) * scale)


def test_u16_upload_equals_fp64_upload_on_a_clipping_shape():
    w, h = 75, 53
    gray, depth = ex.frame(w, h)
    scale = 1.0 / 5000.0
    d16 = np.rint(depth * 5000.0).astype(np.uint16)
    d16[0, 0], d16[h - 1, w - 1], d16[h - 1, 0] = 65535, 1, 0
    nl = ex.num_levels(w, h)
    ncfg, ocfg = _cfgs(nl)
    d64 = d16.astype(np.float64) * scale
    _, d0p = oracle.build_source_pyramids(gray, d64, ocfg)
    with _engine(ncfg, 2, w, h) as e:
        e.upload_frame_u16(0, gray, d16, scale)
        e.upload_frame(1, gray, d64)
        for level in range(nl):
            for a, b in zip(e.get_level_planes(0, level), e.get_level_planes(1, level)):
                assert _same_bits(a, b), level
            assert _same_bits(e.get_level_planes(0, level)[1], d0p[level]), level


@pytest.mark.parametrize("w,h", [(75, 53), (13, 31)])
def test_batched_upload_on_clipping_shapes(w, h):
    """Five different frames in one upload_frames call (blockIdx.z = 0..4) against the same frames one at a time and
    against the oracle; source-only and target-only batches write their planes and the same bits."""
    F = 5
    frames = [ex.frame(w, h, seed) for seed in range(F)]
    gray, depth = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    nl = ex.num_levels(w, h)
    ncfg, ocfg = _cfgs(nl)
    with _engine(ncfg, 4 * F, w, h) as e:
        e.upload_frames(0, gray, depth)
        for f in range(F):
            e.upload_frame(F + f, gray[f], depth[f])
        e.upload_frames(2 * F, gray, depth, roles=native.ROLE_SOURCE)
        e.upload_frames(3 * F, gray, None, roles=native.ROLE_TARGET)
        for f in range(F):
            expect = _oracle_planes(gray[f], depth[f], ocfg)
            for level in range(nl):
                batched = e.get_level_planes(f, level)
                single = e.get_level_planes(F + f, level)
                src = e.get_level_planes(2 * F + f, level)
                tgt = e.get_level_planes(3 * F + f, level)
                for p, name in enumerate("I D GX GY".split()):
                    assert _same_bits(batched[p], expect[level][p]), (f, level, name)
                    assert _same_bits(single[p], expect[level][p]), (f, level, name)
                assert _same_bits(src[0], expect[level][0]) and _same_bits(src[1], expect[level][1]), (f, level)
                for p in (0, 2, 3):
                    assert _same_bits(tgt[p], expect[level][p]), (f, level, p)


def test_non_finite_depth_stays_where_its_taps_are():
    """NaN and +inf at a corner, on the last row and on the last column of 75x53: the depth planes equal the oracle's bit
    for bit, NaN positions included, and only the pixels whose taps (by the exact reference's footprint) touch a planted
    pixel differ from the clean upload."""
    w, h = 75, 53
    gray, depth = ex.frame(w, h)
    planted = {(0, 0): np.inf, (h - 1, w - 1): np.nan, (h - 1, 10): np.inf, (h - 2, 31): np.nan, (20, w - 1): np.nan,
               (41, w - 1): np.inf}
    bad = depth.copy()
    for (y, x), v in planted.items():
        bad[y, x] = v
    nl = ex.num_levels(w, h)
    ncfg, ocfg = _cfgs(nl)
    _, d0p = oracle.build_source_pyramids(gray, bad, ocfg)
    with _engine(ncfg, 2, w, h) as e:
        e.upload_frame(0, gray, depth)
        e.upload_frame(1, gray, bad)
        for level in range(nl):
            clean = e.get_level_planes(0, level)
            got = e.get_level_planes(1, level)
            assert _same_bits(got[1], d0p[level]), level
            for p in (0, 2, 3):
                assert _same_bits(got[p], clean[p]), (level, p)
            lw, lh = ex.level_size(w, h, level)
            xt, yt = ex.resize_taps(w, lw, level), ex.resize_taps(h, lh, level)
            touched = np.zeros((lh, lw), dtype=bool)
            for dy in range(lh):
                for dx in range(lw):
                    touched[dy, dx] = any((y, x) in planted for y, _ in yt[dy] for x, _ in xt[dx])
            assert not np.isfinite(got[1][touched]).any(), level
            assert np.isfinite(got[1][~touched]).all(), level
            assert np.array_equal(got[1][~touched].view(np.uint64), clean[1][~touched].view(np.uint64)), level


@pytest.mark.parametrize("w,h", [(5, 7), (13, 31), (75, 53)])
def test_biobjective_target_planes(w, h):
    """Depth-gradient planes against the exact Scharr of depth * (1/max_depth) and the oracle's bits; the gain against the
    bi-objective checker and the exact quotient.  Level sizes n from 1 (the top of 5x7) to 3975, no multiple of 256."""
    gray, depth = ex.frame(w, h)
    depth = np.where(depth == 0.0, 0.7, depth)                   # a mean of positive depths
    nl = ex.num_levels(w, h)
    ncfg, ocfg = _cfgs(nl)
    tp = ref.target_planes(gray, depth, ocfg, 5.0)
    worst = worst_gain = 0.0
    sizes = []
    with _engine(ncfg, 1, w, h, objective=native.OBJECTIVE_BIOBJECTIVE) as e:
        e.set_depth_range(0.3, 5.0)
        e.upload_frame(0, gray, depth, native.ROLE_TARGET)
        for level in range(nl):
            i1, d1, _, _ = e.get_level_planes(0, level)
            assert _same_bits(i1, tp["i1"][level]) and _same_bits(d1, tp["d1"][level]), level
            n = d1.size
            sizes.append(n)
            dgx, dgy = e.get_level_depth_gradients(0, level)
            assert _same_bits(dgx, tp["dgx"][level]) and _same_bits(dgy, tp["dgy"][level]), level
            gx, mx, gy, my = ex.scharr(ex.to_plane(d1), ex.GRAD_SCALES[level], pre=Fraction(1, 5))
            for g, val, mag in ((dgx, gx, mx), (dgy, gy, my)):
                r = ex.worst_ratio(g, val, mag)
                worst = max(worst, r)
                assert r <= ex.ROUNDINGS_DEPTH_SCHARR, (level, r)
            gain = e.get_level_depth_gain(0, level)
            exact_gain = ex.depth_gain(ex.to_plane(i1), ex.to_plane(d1))
            r = float(abs(Fraction(gain) - exact_gain) / (ex.U * exact_gain))
            worst_gain = max(worst_gain, r)
            assert r <= ex.roundings_gain(n), (level, r, ex.roundings_gain(n))
            # the checker's numpy means: any summation order of n terms is within (n - 1) u, one division each, one quotient
            assert abs(gain - tp["gain"][level]) <= (ex.roundings_gain(n) + 2 * n + 1) * 2.0 ** -53 * tp["gain"][level], level
    assert sizes[-1] <= 2 and all(n % 256 for n in sizes)
    assert (w, h) != (5, 7) or sizes[-1] == 1
    print(f"bi-objective {w}x{h}: level sizes {sizes}; depth Scharr worst {worst:.3f} u*M (bound {ex.ROUNDINGS_DEPTH_SCHARR}); "
          f"gain worst {worst_gain:.3f} u (bound {ex.roundings_gain(sizes[0])} at n = {sizes[0]})")


def test_too_many_levels_are_refused_and_the_engine_lives_on():
    gray, depth = ex.frame(2, 3)
    with odometry.AlignmentEngine(0) as e:
        for (w, h), nl in (((1, 1), 2), ((2, 3), 3)):
            assert ex.num_levels(w, h) == nl - 1
            e.set_config(_cfgs(nl)[0])
            with pytest.raises(native.PhovoError) as ei:
                e.reserve_frames(1, w, h)
            assert ei.value.status == native.E_SHAPE
        ncfg, ocfg = _cfgs(2)
        e.set_config(ncfg)
        e.set_build_all_levels(True)
        e.reserve_frames(1, 2, 3)
        e.upload_frame(0, gray, depth)
        expect = _oracle_planes(gray, depth, ocfg)
        for level in range(2):
            assert e.level_size(level) == ex.level_size(2, 3, level)
            for g, o in zip(e.get_level_planes(0, level), expect[level]):
                assert _same_bits(g, o), level
