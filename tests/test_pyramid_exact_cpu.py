"""The CPU oracle's pyramid producers against the exact reference tests/pyramid_exact.py, at the shapes that clip.

oracle/phovo_oracle.c and csrc/pyramid_kernels.hip were written operation for operation from one restatement, so their
bit equality says nothing about a mistake the two share.  Here the oracle is held to the definition of each producer in
rational arithmetic: level sizes exactly, every plane within (roundings on the longest path) * 2^-53 * M of the exact value
(the counts are derived in pyramid_exact.py's docstring; nothing is measured into them).  tests/test_gpu_pyramid_edges.py
holds the device to the same reference at the same shapes.  Every test prints the worst ratio it met, in units of 2^-53 * M.
"""
from fractions import Fraction

import numpy as np
import pytest

import pyramid_exact as ex

from oracle import oracle

SHAPE_IDS = [f"{w}x{h}" for w, h in ex.SHAPES]
BLUR_IDS = [f"{w}x{h}-{'_'.join(map(str, b))}" for w, h, b in ex.BLUR_CASES]


def _cfg(nl, blur=None):
    return oracle.make_config(num_levels=nl, blur=list(blur) if blur else [0] * nl, grad_scale=ex.GRAD_SCALES[:nl],
                              max_iter=[1] * nl)


@pytest.mark.parametrize("w,h", ex.SHAPES, ids=SHAPE_IDS)
def test_level_sizes_are_round_half_even(w, h):
    nl = ex.num_levels(w, h)
    assert nl >= 1
    for level in range(nl + 2):                                  # the first empty levels too
        assert oracle.level_size(w, h, level) == ex.level_size(w, h, level), level


def test_the_shapes_tell_half_even_from_half_up():
    assert ex.level_size(75, 53, 1) == (38, 26) and ex.level_size(77, 51, 1) == (38, 26)       # half-up: 39 x 26
    assert ex.level_size(511, 5, 1) == (256, 2) and ex.level_size(255, 2, 2)[1] == 0
    assert [ex.num_levels(w, h) for w, h in ex.SHAPES] == [1, 2, 2, 4, 5, 7, 7, 5, 2, 3, 4, 4, 5]


@pytest.mark.parametrize("w,h", ex.SHAPES, ids=SHAPE_IDS)
def test_oracle_resize_against_exact(w, h):
    gray, depth = ex.frame(w, h)
    nl = ex.num_levels(w, h)
    cfg = _cfg(nl)
    i0p, d0p = oracle.build_source_pyramids(gray, depth, cfg)
    np.testing.assert_array_equal(i0p[0], ex.intensity_plane(gray))
    levels = ex.exact_levels(w, h)
    worst = 0.0
    for level in range(nl):
        for got, (val, mag) in ((i0p[level], levels[level]["i"]), (d0p[level], levels[level]["d"])):
            assert got.shape == ex.level_size(w, h, level)[::-1]
            r = ex.worst_ratio(got, val, mag)
            worst = max(worst, r)
            assert r <= ex.roundings_resize(level), (level, r)
    print(f"resize {w}x{h}: worst |oracle - exact| = {worst:.3f} u*M (bound {ex.ROUNDINGS_RESIZE_1} / {ex.ROUNDINGS_RESIZE})")


def test_oracle_resize_of_a_signed_plane_against_exact():
    """Mixed signs: M = sum |c * tap| is larger than |exact| and the bound is on M."""
    w, h = 13, 31
    plane = np.random.RandomState(5).uniform(-1.0, 1.0, size=(h, w))
    p = ex.to_plane(plane)
    worst = 0.0
    for level in range(1, ex.num_levels(w, h)):
        val, mag = ex.resize(p, level)
        r = ex.worst_ratio(oracle.resize_level(plane, level), val, mag)
        worst = max(worst, r)
        assert r <= ex.roundings_resize(level), (level, r)
    zero = np.zeros((h, w))
    assert not oracle.resize_level(zero, 1).any() and not oracle.resize_level(zero, 3).any()     # M = 0: exactly 0
    print(f"resize, signed 13x31: worst {worst:.3f} u*M")


@pytest.mark.parametrize("w,h", ex.SHAPES, ids=SHAPE_IDS)
def test_oracle_scharr_against_exact(w, h):
    """Scharr of the oracle's own level planes (the doubles as they are), with the per-level scale; depth * (1/max_depth)
    with the scale as the bi-objective target builds it."""
    gray, depth = ex.frame(w, h)
    nl = ex.num_levels(w, h)
    cfg = _cfg(nl)
    i1p, gxp, gyp = oracle.build_target_pyramids(gray, cfg)
    _, d1p = oracle.build_source_pyramids(gray, depth, cfg)
    worst = worst_d = 0.0
    for level in range(nl):
        scale = ex.GRAD_SCALES[level]
        gx, mx, gy, my = ex.scharr(ex.to_plane(i1p[level]), scale)
        for got, val, mag in ((gxp[level], gx, mx), (gyp[level], gy, my)):
            r = ex.worst_ratio(got, val, mag)
            worst = max(worst, r)
            assert r <= ex.ROUNDINGS_SCHARR, (level, r)
        if w == 1:
            assert not gxp[level].any()                              # one column: both x taps are the pixel itself
        ogx, ogy = oracle.scharr(d1p[level] * (1.0 / 5.0), scale)
        gx, mx, gy, my = ex.scharr(ex.to_plane(d1p[level]), scale, pre=Fraction(1, 5))
        for got, val, mag in ((ogx, gx, mx), (ogy, gy, my)):
            r = ex.worst_ratio(got, val, mag)
            worst_d = max(worst_d, r)
            assert r <= ex.ROUNDINGS_DEPTH_SCHARR, (level, r)
    print(f"Scharr {w}x{h}: worst {worst:.3f} u*M (bound {ex.ROUNDINGS_SCHARR}); of depth/max_depth {worst_d:.3f} u*M "
          f"(bound {ex.ROUNDINGS_DEPTH_SCHARR})")


@pytest.mark.parametrize("w,h,blur", ex.BLUR_CASES, ids=BLUR_IDS)
def test_oracle_blur_against_exact(w, h, blur):
    """GaussianBlur twice on every level, kernels wider than the image (reflect-101 bounces more than once), the largest
    accepted size 63, and the level-0 alias: a level-0 blur feeds every later level."""
    assert len(blur) == ex.num_levels(w, h)
    gray, _ = ex.frame(w, h)
    i1p, _, _ = oracle.build_target_pyramids(gray, _cfg(len(blur), blur))
    worst = []
    for level, (val, mag, count) in enumerate(ex.exact_blur_case(w, h, blur)):
        r = ex.worst_ratio(i1p[level], val, mag)
        worst.append((round(r, 2), round(float(count), 1)))
        assert r <= count, (level, r, float(count))
    print(f"blur {w}x{h} {blur}: per level (worst u*M, bound) {worst}")


def test_blur_coefficients_and_border():
    """The reference itself: coefficients sum to 1 and are symmetric; reflect-101 is gfedcb|abcdefgh|gfedcba."""
    for k in (1, 3, 5, 9, 21, 63):
        g = ex.gaussian_coefficients(k)
        assert sum(g) == 1 and all(g[i] == g[k - 1 - i] for i in range(k)) and g[k // 2] == max(g)
    assert [ex.reflect101(p, 4) for p in range(-7, 11)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert [ex.reflect101(p, 1) for p in (-3, 0, 5)] == [0, 0, 0]
    assert [ex.reflect101(p, 2) for p in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert ex.roundings_blur(3) < 72 and ex.roundings_blur(63) < 1404 and ex.roundings_blur(1) == 0


def test_these_shapes_reach_the_unverified_branches():
    """The tautology check: the branches tagged UNVERIFIED-vs-OpenCV -- [0] the clipped 2x2 block, [1] the tap clamped at
    scales >= 4, [2] the blur -- are the ones these shapes and blur cases run.  [1] needs a size whose quotient by 2^L ends
    in exactly one half and rounds up (pyramid_exact.SHAPES): only the two shapes added for it reach it."""
    oracle.unverified_hits(reset=True)
    hits = {}
    for w, h in ex.SHAPES:
        gray, depth = ex.frame(w, h)
        oracle.build_source_pyramids(gray, depth, _cfg(ex.num_levels(w, h)))
        hits[(w, h)] = oracle.unverified_hits(reset=True)
    assert all(v[2] == 0 for v in hits.values())
    assert hits[(75, 53)][0] == 2 * 26                            # 75 -> 38 keeps the odd column (26 rows, two planes), 53 -> 26 drops the odd row
    assert hits[(77, 51)][0] == 2 * 38                            # 77 -> 38 drops the odd column, 51 -> 26 keeps the odd row
    assert hits[(257, 9)][0] == 0 and hits[(1, 1)] == (0, 0, 0)
    assert [s for s in ex.SHAPES if hits[s][1] > 0] == ex.CLAMPED_TAP_SHAPES
    assert hits[(6, 14)][1] == 2 * (1 + 4)                        # level 2 (2 x 4): the last row once, the last column on 4 rows
    for w, h, blur in ex.BLUR_CASES:
        oracle.build_target_pyramids(ex.frame(w, h)[0], _cfg(len(blur), blur))
    assert oracle.unverified_hits(reset=True)[2] > 0
    total = [sum(v[b] for v in hits.values()) for b in range(2)]
    assert total[0] > 0 and total[1] > 0, total
