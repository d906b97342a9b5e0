"""Exact reference of the pyramid producers (level size, resize from level 0, Scharr, Gaussian blur, the bi-objective
target planes), in rational arithmetic.  Test infrastructure, not collected as tests.

Written from the DEFINITION of each producer, not from oracle/phovo_oracle.c: every input is the double it is given, taken
as a fractions.Fraction, and every result is the exact value of a linear form  sum_t c_t * tap_t  together with its
magnitude  M = sum_t |c_t * tap_t|.  A double-precision producer that evaluates the same form is then held to

    |computed - exact|  <=  ROUNDINGS * 2^-53 * M,

ROUNDINGS being the number of roundings on the longest path from an input to the output of the producer's formula
(Jeannerod and Rump, "Improved error bounds for inner products in floating-point arithmetic", SIAM J. Matrix Anal. Appl.
34, 2013: n roundings in round-to-nearest cost at most n*u, with no higher-order term, as long as nothing underflows).
Where M = 0 the bound is 0 and the result must be exactly 0.  The counts:

  resize, level 1     3   (((a + b) + c) + d) * 0.25: three additions; the scaling by 1/4 (or, for a clipped block, the
                          division by 1 or 2 after one addition) is exact.
  resize, level >= 2  2   a*0.5 + b*0.5 along the row, then top*0.5 + bot*0.5: products with 0.5 are exact, the longest
                          path crosses two additions.
  Scharr              5   fl(3*scale) or fl(10*scale); one addition in the [-1, 0, 1] filter (or two products-and-sums of
                          the smoothing filter); one sum of the outer rows; one product; one last addition -- five on
                          either plane.
  depth Scharr        7   Scharr of depth * (1/max_depth): fl(1/max_depth) and the product with the depth come on top.
  depth gain          2*(ceil(n/256) + 8) + 1
                          each of the two means is a sum of n terms in 256 strided partial sums (ceil(n/256) - 1
                          additions), a tree of 8 levels and one division by n; one last division.
  blur, k <= 1        0   the kernel is [1]: every product is exact and nothing is added.
  blur, k >= 3        4 * (2*k + 4*a + 11) + 1,   a = ((k - 1)/2)^2 / 18
                          GaussianBlur twice = four passes (rows, columns, rows, columns).  A pass costs at most k
                          roundings of its own (row pass: one product and k - 1 additions; column pass: (k - 1)/2 + 2)
                          and carries the error of its coefficients: a coefficient is exp(arg_i) / sum_j exp(arg_j), where
                          a relative error d of arg_i moves exp by |arg_i| * d.  Numerator: three roundings in the
                          producer's argument and one in this file's, each times |arg_i| <= a; exp itself within one
                          ulp = 2u on either side: 4*a + 4.  Denominator: the same perturbations averaged with the
                          coefficients as weights, 4*mean(|arg|) + 4 <= 4 * (sigma^2/18 = 1/2) + 4 = 6; k - 1 additions;
                          one reciprocal.  One product.  Together 4*a + k + 11 per pass.  The + 1 absorbs every second-order
                          term of chaining the passes (n^2 u^2 < u for n < 2^26).
  chained producers   the counts add, plus 1 for the second-order terms (level-0 blur, resize, level blur).

The blur count is far above what is measured (12.6 u on non-negative images, k up to 63; the count is 70 at k = 3 and 1403
at k = 63, so more than four times that figure): the longest path runs through the outermost tap, whose exponent 53.4
at k = 63 multiplies every rounding of the argument, and through k additions per pass, while the measured error is carried
by the few central taps that hold nearly all of the weight and adds up like a random walk.  The count bounds the worst
image (all weight under the outermost taps), which no test image is; the mistakes the bound is there to catch -- a wrong
border, a wrong or unnormalised coefficient -- are larger than 1e-3 of M.
"""
import functools
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
SIGMA2 = 9                                   # GaussianBlur(..., sigma = 3)

ROUNDINGS_RESIZE_1 = 3
ROUNDINGS_RESIZE = 2
ROUNDINGS_SCHARR = 5
ROUNDINGS_DEPTH_SCHARR = 7


def roundings_resize(level):
    return 0 if level == 0 else ROUNDINGS_RESIZE_1 if level == 1 else ROUNDINGS_RESIZE


def roundings_blur(k):
    if k <= 1:
        return 0
    a = Fraction(((k - 1) // 2) ** 2, 2 * SIGMA2)
    return 4 * (2 * k + 4 * a + 11) + 1


def roundings_chain(*counts):
    """Producers applied one after the other."""
    counts = [c for c in counts if c]
    return sum(counts) + (1 if len(counts) > 1 else 0)


def roundings_gain(n):
    return 2 * (-(-n // 256) + 8) + 1


# ---------------------------------------------------------------------------------------------------------------------
# planes of Fractions: a plane is a list of rows
# ---------------------------------------------------------------------------------------------------------------------
def to_plane(a):
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 2 and np.all(np.isfinite(a))
    return [[Fraction(float(v)) for v in row] for row in a]


def magnitude_of(plane):
    return [[abs(v) for v in row] for row in plane]


def _nonneg(plane):
    return all(v >= 0 for row in plane for v in row)


def level_size(w, h, level):
    """round-half-even of w / 2^level: Python's round() of a Fraction."""
    return round(Fraction(w, 2 ** level)), round(Fraction(h, 2 ** level))


def num_levels(w, h):
    """As many levels as give non-empty planes."""
    n = 0
    while min(level_size(w, h, n)) > 0:
        n += 1
    return n


def _apply(src, xtaps, ytaps):
    """out[y][x] = sum over ytaps[y] x xtaps[x] of cy * cx * src: along the rows first, then along the columns."""
    rows = [[sum(c * r[i] for i, c in taps) for taps in xtaps] for r in src]
    return [[sum(c * rows[j][x] for j, c in taps) for x in range(len(xtaps))] for taps in ytaps]


def _apply_nonneg(plane, mag, xtaps, ytaps):
    """Non-negative coefficients: the magnitude is the same form on `mag`, and where `mag` is the plane itself (a
    non-negative plane) the two coincide and are computed once."""
    val = _apply(plane, xtaps, ytaps)
    return val, (val if mag is plane else _apply(mag, xtaps, ytaps))


# ---------------------------------------------------------------------------------------------------------------------
# resize from level 0
# ---------------------------------------------------------------------------------------------------------------------
def resize_taps(n, out_n, level):
    """Along one axis of n pixels: for each of the out_n output pixels the list of (source index, weight).
    Level 1: the part of the pair {2d, 2d + 1} that lies inside, equally weighted (the mean of what is inside).
    Level >= 2: linear interpolation at (d + 1/2) * 2^level - 1/2, tap indices clamped to the last pixel."""
    s = 2 ** level
    out = []
    for d in range(out_n):
        if level == 0:
            taps = {d: Fraction(1)}
        elif level == 1:
            inside = [i for i in (2 * d, 2 * d + 1) if i < n]
            taps = {i: Fraction(1, len(inside)) for i in inside}
        else:
            p = (d + Fraction(1, 2)) * s - Fraction(1, 2)
            i0 = math.floor(p)
            f = p - i0
            taps = {}
            for i, c in ((i0, 1 - f), (i0 + 1, f)):
                i = min(max(i, 0), n - 1)
                taps[i] = taps.get(i, 0) + c
        out.append(sorted(taps.items()))
    return out


def resize(plane, level, mag=None):
    """Level `level` of a level-0 plane: (value, magnitude)."""
    h, w = len(plane), len(plane[0])
    lw, lh = level_size(w, h, level)
    assert lw > 0 and lh > 0
    mag = plane if mag is None and _nonneg(plane) else magnitude_of(plane) if mag is None else mag
    return _apply_nonneg(plane, mag, resize_taps(w, lw, level), resize_taps(h, lh, level))


# ---------------------------------------------------------------------------------------------------------------------
# borders, Scharr, Gaussian blur
# ---------------------------------------------------------------------------------------------------------------------
def reflect101(p, n):
    """gfedcb|abcdefgh|gfedcba: the mirror about the first and the last pixel, as often as it takes."""
    if n == 1:
        return 0
    p %= 2 * (n - 1)
    return p if p < n else 2 * (n - 1) - p


def _filter_taps(n, kernel):
    """A centred 1-D filter on reflect-101 borders, folded onto the n source pixels."""
    r = (len(kernel) - 1) // 2
    out = []
    for d in range(n):
        taps = {}
        for i, c in enumerate(kernel):
            if c != 0:
                j = reflect101(d - r + i, n)
                taps[j] = taps.get(j, 0) + c
        out.append(sorted(taps.items()))
    return out


def _filter_signed(plane, mag, kx, ky):
    """A separable filter whose coefficients carry signs: the magnitude folds |coefficients| (a tap met twice through the
    border with opposite signs cancels in the value, not in the magnitude)."""
    h, w = len(plane), len(plane[0])
    val = _apply(plane, _filter_taps(w, kx), _filter_taps(h, ky))
    return val, _apply(mag, _filter_taps(w, [abs(c) for c in kx]), _filter_taps(h, [abs(c) for c in ky]))


def scharr(plane, scale, mag=None, pre=1):
    """(gx, gx magnitude, gy, gy magnitude): the 3x3 products of [-1, 0, 1] with scale*[3, 10, 3] (gx: the derivative
    along x; gy: along y), reflect-101 borders, of pre * plane (pre: the exact factor of the bi-objective depth planes)."""
    scale = Fraction(scale) * Fraction(pre)
    deriv = [Fraction(-1), Fraction(0), Fraction(1)]
    smooth = [3 * scale, 10 * scale, 3 * scale]
    mag = magnitude_of(plane) if mag is None else mag
    gx, mx = _filter_signed(plane, mag, deriv, smooth)
    gy, my = _filter_signed(plane, mag, smooth, deriv)
    return gx, mx, gy, my


@functools.lru_cache(maxsize=None)
def gaussian_coefficients(k):
    """exp(-x^2 / (2*9)) at x = i - (k - 1)/2 from math.exp, as Fractions, normalised exactly."""
    e = []
    for i in range(k):
        x = Fraction(2 * i - (k - 1), 2)
        e.append(Fraction(math.exp(float(-(x * x) / (2 * SIGMA2)))))
    s = sum(e)
    return tuple(c / s for c in e)


def blur_twice(plane, k, mag=None):
    """GaussianBlur(k x k, sigma 3) applied twice: rows then columns, reflect-101, the whole filter twice."""
    mag = plane if mag is None and _nonneg(plane) else magnitude_of(plane) if mag is None else mag
    if k <= 1:
        return plane, mag
    h, w = len(plane), len(plane[0])
    g = list(gaussian_coefficients(k))
    xt, yt = _filter_taps(w, g), _filter_taps(h, g)
    for _ in range(2):
        shared = mag is plane
        plane, mag = _apply_nonneg(plane, mag, xt, yt)
        if shared:
            mag = plane
    return plane, mag


def intensity_pyramid(plane0, blur):
    """The intensity pyramid under blur sizes `blur` (one per level, 0 = none): per level (value, magnitude, roundings).
    A level-0 blur is in place: every later level is resized from the blurred level 0."""
    base, base_mag, base_count = plane0, None, 0
    out = []
    for level, k in enumerate(blur):
        if level == 0:
            v, m = blur_twice(plane0, k)
            if k > 0:
                base, base_mag, base_count = v, m, roundings_blur(k)
            out.append((v, m, roundings_blur(k) if k > 0 else 0))
            continue
        v, m = resize(base, level, base_mag)
        v, m = blur_twice(v, k, m)
        out.append((v, m, roundings_chain(base_count, roundings_resize(level), roundings_blur(k))))
    return out


def depth_gain(intensity, depth):
    """mean(I) / mean(D) of one level.  The two means of non-negative planes carry no cancellation, so the magnitude of
    the quotient is the quotient itself."""
    n = len(intensity) * len(intensity[0])
    assert _nonneg(intensity) and _nonneg(depth)
    mi = sum(v for r in intensity for v in r) / n
    md = sum(v for r in depth for v in r) / n
    return mi / md


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, exact, mag):
    """max over the plane of |got - exact| / (2^-53 * M), in units of u; where M = 0 the value must be exactly 0
    (anything else returns inf)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (len(exact), len(exact[0])), (got.shape, len(exact), len(exact[0]))
    assert np.all(np.isfinite(got))
    worst = Fraction(0)
    for y, row in enumerate(exact):
        for x, e in enumerate(row):
            err = abs(Fraction(float(got[y, x])) - e)
            m = mag[y][x]
            if m == 0:
                if err != 0:
                    return math.inf
            else:
                worst = max(worst, err / (U * m))
    return float(worst)


# ---------------------------------------------------------------------------------------------------------------------
# the shapes and inputs the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------
# (width, height): 75 -> 38 and 77 -> 38, 53 -> 26 and 51 -> 26 tell half-even from half-up; 511 -> 256 ends on a block edge.
# A tap is clamped to the last row or column at a scale >= 4 only where size / 2^L ends in exactly one half and is
# rounded UP to the even neighbour (the last output pixel then samples at size - 1/2): 6 / 4 and 12 / 8 -> 2, 14 / 4 and
# 28 / 8 -> 4.  None of the first eleven shapes does that, so 6x14 and 28x12 stand beside them.
SHAPES = [(1, 1), (2, 3), (3, 2), (5, 7), (13, 31), (75, 53), (77, 51), (257, 9), (255, 2), (256, 3), (511, 5),
          (6, 14), (28, 12)]
CLAMPED_TAP_SHAPES = [(6, 14), (28, 12)]
GRAD_SCALES = [0.0625, 0.125, 0.03, 0.0625, 0.1, 0.25, 0.07]           # per level; 0.03, 0.1 and 0.07 are no powers of two

# (width, height, blur size per level): every level of the shape, a different size on each, with and without the
# level-0 alias; the sizes 1, 3, 5, 9, 21 and 63, all but the smallest wider than the image
BLUR_CASES = [
    (1, 5, (63,)), (1, 5, (5,)), (1, 5, (21,)),
    (5, 1, (9,)), (5, 1, (63,)), (5, 1, (3,)),
    (2, 2, (63, 3)), (2, 2, (0, 5)),
    (4, 3, (5, 9, 3)), (4, 3, (0, 63, 21)), (4, 3, (1, 21, 63)),
    (11, 6, (3, 5, 9, 21)), (11, 6, (63, 21, 1, 3)), (11, 6, (0, 9, 63, 5)), (11, 6, (21, 63, 5, 9)),
]


def frame(w, h, seed=0):
    """A seeded frame: gray u8 with 0 and 255 present where there is room, and a positive fp64 depth with zeros (holes)."""
    rs = np.random.RandomState(1000 * w + h + 7919 * seed)
    gray = rs.randint(0, 256, size=(h, w)).astype(np.uint8)
    depth = rs.uniform(0.4, 4.6, size=(h, w))
    depth[rs.uniform(size=(h, w)) < 0.05] = 0.0
    if w * h >= 4:
        gray.flat[0], gray.flat[-1] = 255, 0
    return gray, depth


def intensity_plane(gray):
    """convertTo(fp64, 1./255): the double nearest to v * fl(1/255), which is the input of everything behind it."""
    return np.asarray(gray, dtype=np.float64) * (1.0 / 255)


@functools.lru_cache(maxsize=None)
def exact_levels(w, h, seed=0):
    """Per level of frame(w, h, seed), without blur: dict(i=(value, magnitude), d=(value, magnitude)), computed once."""
    gray, depth = frame(w, h, seed)
    i0, d0 = to_plane(intensity_plane(gray)), to_plane(depth)
    return [dict(i=resize(i0, level), d=resize(d0, level)) for level in range(num_levels(w, h))]


@functools.lru_cache(maxsize=None)
def exact_blur_case(w, h, blur, seed=0):
    gray, _ = frame(w, h, seed)
    return intensity_pyramid(to_plane(intensity_plane(gray)), blur)
