"""Warp problems whose answer is known without running a warp, and the draws of the warp sweep.  No device, no oracle.

The exact problems.  With fx = fy = 64 * 2^level, a principal point that is a multiple of 2^level, depths that are powers
of two, R = I and dyadic translations, every product, the division and every sum of phovo::warpImage
(phovo/include/CPhotoconsistencyOdometry.h:73-134) is exact in binary64.  The projection of source pixel (r, c) at depth d
under the translation t is then the rational number

    column' = ((c - ox) d / 64 + tx) 64 / (d + tz) + ox            row' likewise with r, oy, ty,

which this module evaluates with fractions.Fraction from the pinhole model, cuts toward zero (the reference's
static_cast<int>), and places by numpy indexing with the largest source index winning (the reference overwrites in raster
order).  Nothing here runs floating-point projection arithmetic, so a misreading that the kernel and the oracle share is
not shared by these expectations; tests/test_warp_cases_cpu.py holds them to the oracle and to the reference build.

What the reference does with a source pixel, restated once (the only rules used below):
  * depth > 0 or the pixel is skipped (:107) -- so 0.0, -0.0, negatives and NaN are skipped, +inf and subnormals are not;
  * no test on the transformed Z: a point behind the camera is projected through the centre and written where it lands;
  * the coordinate is cast with static_cast<int>: toward zero, so (-1, 0) is column / row 0 and exactly -1.0 is outside;
  * a coordinate that is not finite or beyond int is undefined there; the project (kernel and oracle) drops the pixel;
  * later raster writers overwrite earlier ones; where nothing lands the image is 0.
"""
import math
from fractions import Fraction

import numpy as np

MAX_LEVELS = 16                      # PHOVO_MAX_LEVELS (include/phovo_hip.h)
F = 64                               # the effective focal length of every exact problem
GRID_STRIDE = 4096 * 256             # pixels per trip of the kernels' grid-stride loop (warp_kernels.hip: 4096 workgroups of 256)
BIG_W, BIG_H = 1025, 1024            # the smallest convenient image above GRID_STRIDE pixels: 1,049,600
INT_LIMIT = 2 ** 31

NO_REFERENCE_BUILD = ("inf_depth", "z_zero", "z_tiny")     # the reference's cast is undefined there: oracle only


def gray_ramp(w, h):
    """1 + index % 251: neighbours differ (rows too, unless w is a multiple of 251) and no pixel is 0."""
    return (1 + np.arange(w * h) % 251).astype(np.uint8).reshape(h, w)


def passes_gate(d):
    return bool(d > 0)               # False for 0.0, -0.0, negatives and NaN


def exact_coordinate(i, o, d, t, tz):
    """The projected column (row) of source column (row) i as a Fraction; None where it does not exist (Z' = 0, d = inf)."""
    if math.isinf(d):
        return None
    d, t, tz, o = Fraction(d), Fraction(t), Fraction(tz), Fraction(o)
    z = d + tz
    if z == 0:
        return None
    return ((i - o) * d / F + t) * F / z + o


def cell(v, n):
    """static_cast<int> of an exact coordinate; -1 where the pixel is dropped."""
    if v is None or abs(v) >= INT_LIMIT:
        return -1
    k = math.trunc(v)                # toward zero
    return k if 0 <= k < n else -1


def place(gray, targets):
    """The warped image from per-source flat target indices (-1 = dropped): the largest source index on a target wins.
    Returns (image, owner map with -1 where nothing landed)."""
    h, w = gray.shape
    t = np.asarray(targets).reshape(-1)
    src = np.flatnonzero(t >= 0)                                   # ascending = raster order
    owner = np.full(w * h, -1, dtype=np.int64)
    if src.size:
        cells, first_from_the_back = np.unique(t[src][::-1], return_index=True)
        owner[cells] = src[::-1][first_from_the_back]              # the last raster writer of every target
    out = np.zeros(w * h, dtype=np.uint8)
    out[owner >= 0] = gray.reshape(-1)[owner[owner >= 0]]
    return out.reshape(h, w), owner.reshape(h, w)


class Problem:
    """One exact problem: inputs for phovo_warp_image, the expected image, its owner map and the facts that say the
    problem reached its edge (`reached`: name -> bool, every one computed in exact arithmetic)."""

    def __init__(self, name, kind, w, h, ox, oy, t, dz=1.0, level=0, specials=(), reached=None):
        self.name, self.kind, self.w, self.h, self.level = name + (f"_dz{dz:g}" if dz != 1.0 else ""), kind, w, h, level
        self.ox, self.oy, self.dz = ox, oy, dz
        self.t = tuple(float(Fraction(v) * Fraction(dz)) for v in t)          # translations are given in units of dz
        assert all(Fraction(a) == Fraction(v) * Fraction(dz) for a, v in zip(self.t, t))     # representable: dyadic
        s = float(2 ** level)
        self.K = np.array([[F * s, 0.0, ox * s], [0.0, F * s, oy * s], [0.0, 0.0, 1.0]])
        self.rt = np.eye(4)
        self.rt[:3, 3] = self.t
        self.gray = gray_ramp(w, h)
        self.depth = np.full((h, w), float(dz))
        self.specials = tuple(specials)
        for r, c, d in self.specials:
            self.depth[r, c] = d
        self.cols = [exact_coordinate(c, ox, dz, self.t[0], self.t[2]) for c in range(w)]
        self.rows = [exact_coordinate(r, oy, dz, self.t[1], self.t[2]) for r in range(h)]
        tc = np.array([cell(v, w) for v in self.cols], dtype=np.int64)
        tr = np.array([cell(v, h) for v in self.rows], dtype=np.int64)
        targets = np.where((tr[:, None] >= 0) & (tc[None, :] >= 0), tr[:, None] * w + tc[None, :], -1)
        for r, c, d in self.specials:
            targets[r, c] = self.special_target(r, c, d)
        self.targets = targets
        self.expected, self.owner = place(self.gray, targets)
        self.collisions = int(np.count_nonzero(targets >= 0) - np.count_nonzero(self.owner >= 0))
        self.reached = dict(reached(self) if reached else {})

    def special_target(self, r, c, d):
        if not passes_gate(d):
            return -1
        a = cell(exact_coordinate(c, self.ox, d, self.t[0], self.t[2]), self.w)
        b = cell(exact_coordinate(r, self.oy, d, self.t[1], self.t[2]), self.h)
        return b * self.w + a if a >= 0 and b >= 0 else -1

    @property
    def reference_build_defined(self):
        return self.kind not in NO_REFERENCE_BUILD

    def __repr__(self):
        return self.name


def _centre(w, h):
    return w // 2, h // 2


# ------------------------------------------------------------------------------------------------------------------------
# constructions
# ------------------------------------------------------------------------------------------------------------------------
def identity(w, h, level=0, dz=1.0):
    ox, oy = _centre(w, h)
    return Problem(f"identity_{w}x{h}_L{level}", "identity", w, h, ox, oy, (0, 0, 0), dz, level,
                   reached=lambda p: {"every pixel maps to itself":
                                      np.array_equal(p.targets.reshape(-1), np.arange(w * h))})


def shift(w, h, sx, sy, level=0, dz=1.0):
    """tx = -sx dz / 64: every column moves by exactly -sx (rows by -sy).  Halves sit in the middle between two pixels."""
    ox, oy = _centre(w, h)
    sx, sy = Fraction(sx), Fraction(sy)

    def reached(p):
        return {"columns land on c - sx exactly": all(v == c - sx for c, v in enumerate(p.cols)),
                "rows land on r - sy exactly": all(v == r - sy for r, v in enumerate(p.rows)),
                "first or last coordinate is the intended border value":
                    (sx == 0 or p.cols[0] == -sx and p.cols[-1] == w - 1 - sx)
                    and (sy == 0 or p.rows[0] == -sy and p.rows[-1] == h - 1 - sy)}
    return Problem(f"shift_{float(sx):+g}_{float(sy):+g}_{w}x{h}_L{level}", "shift", w, h, ox, oy,
                   (-sx / F, -sy / F, 0), dz, level, reached=reached)


def halving(w, h, level=0, dz=1.0, specials=(), kind="halving", name=None, extra=None):
    """tz = dz: Z' = 2 dz, so column' = (c - ox) / 2 + ox: a 2x2 block of sources per target, odd distances on a half."""
    ox, oy = _centre(w, h)

    def reached(p):
        facts = {"columns land on (c - ox) / 2 + ox exactly":
                 all(v == Fraction(c - ox, 2) + ox for c, v in enumerate(p.cols)),
                 "half-integer coordinates occur on both sides of the principal point":
                     (w < 4 or any(v.denominator == 2 and v < ox for v in p.cols)
                      and any(v.denominator == 2 and v > ox for v in p.cols))}
        if extra:
            facts.update(extra(p))
        return facts
    return Problem(name or f"{kind}_{w}x{h}_L{level}", kind, w, h, ox, oy, (0, 0, 1), dz, level, specials, reached)


def gate(w, h, level=0):
    """The halving problem with the four sources of one target at 0.0, -0.0, -1.0 and NaN: that target stays 0.  The block
    is chosen behind the principal point's own sources in raster order: a `>=` gate would project the zero depths to t, which
    is the principal point, and overwrite the winner there."""
    ox, oy = _centre(w, h)
    r0, c0 = oy + 2, ox + 4                                        # the block (r0, c0) .. (r0 + 1, c0 + 1), target (oy + 1, ox + 2)
    bad = [(r0, c0, -1.0), (r0, c0 + 1, float("nan")), (r0 + 1, c0, -0.0), (r0 + 1, c0 + 1, 0.0)]

    def extra(p):
        tgt = (oy + 1) * w + ox + 2
        block = [(r0 + a) * w + c0 + b for a in (0, 1) for b in (0, 1)]
        plain = halving(w, h, level)
        return {"without the bad depths the four sources share one target":
                    all(plain.targets.reshape(-1)[i] == tgt for i in block),
                "that target is empty": p.expected.reshape(-1)[tgt] == 0 and p.owner.reshape(-1)[tgt] == -1,
                "a zero depth let through would win at the principal point":
                    (r0 + 1) * w + c0 + 1 > p.owner[oy, ox] >= 0}
    return halving(w, h, level, specials=bad, kind="gate", extra=extra)


def inf_depth(w, h, level=0):
    """+inf passes the gate; its coordinates are not finite (0 * inf in Rt * point), so nothing is written for it."""
    ox, oy = _centre(w, h)
    at = (oy + 3, ox + 5)

    def extra(p):
        return {"the pixel is dropped and its block's winner is not it": p.targets[at] == -1}
    return halving(w, h, level, specials=[(at[0], at[1], float("inf"))], kind="inf_depth", extra=extra)


def subnormal_depth(w, h, level=0):
    """2^-1060 passes the gate.  Z' = 2^-1060 + dz, so the pixel lands a hair beyond the principal point: on it, after the
    cast.  It sits right and below of the principal point (the hair is positive) and late in raster order, so it wins there."""
    ox, oy = _centre(w, h)
    at = (h - 1, w - 1)

    def extra(p):
        v = exact_coordinate(at[1], ox, 2.0 ** -1060, 0, 1)
        return {"the coordinate is the principal point plus less than 2^-1000": 0 < v - ox < Fraction(1, 2 ** 1000),
                "it wins at the principal point": p.owner[oy, ox] == at[0] * w + at[1]}
    return halving(w, h, level, specials=[(at[0], at[1], 2.0 ** -1060)], kind="subnormal_depth", extra=extra)


def collapse(w, h, level=0, dz=1.0):
    """tz = 1023 dz: column' = (c - ox) / 1024 + ox, so every pixel lands on one of the four cells around the principal
    point; the winners are the last pixel of each quadrant."""
    ox, oy = _centre(w, h)

    def reached(p):
        cells = {(oy - 1, ox - 1): (oy - 1, ox - 1), (oy - 1, ox): (oy - 1, w - 1),
                 (oy, ox - 1): (h - 1, ox - 1), (oy, ox): (h - 1, w - 1)}
        cells = {k: v for k, v in cells.items() if min(k) >= 0}
        hits = np.bincount(p.targets.reshape(-1), minlength=w * h).reshape(h, w)
        return {"every pixel lands": bool(np.all(p.targets >= 0)),
                "only the cells around the principal point are hit":
                    set(zip(*np.nonzero(hits))) == set(cells),
                "the winners are the last pixels of the quadrants":
                    all(p.owner[k] == v[0] * w + v[1] for k, v in cells.items()),
                "hundreds of sources or all of them on one address":
                    hits.max() >= min(1024, w * h // 4)}
    return Problem(f"collapse_{w}x{h}_L{level}", "collapse", w, h, ox, oy, (0, 0, 1023), dz, level, reached=reached)


def behind(w, h, half=False, level=0, dz=1.0):
    """tz = -2 dz: Z' = -dz < 0.  The reference does not test Z', so the point reflection about the principal point is
    written: column' = 2 ox - c, with tx = dz / 128 half a pixel less (and then cut toward zero, -0.5 to 0)."""
    ox, oy = _centre(w, h)
    s = Fraction(1, 2) if half else Fraction(0)

    def reached(p):
        return {"columns land on 2 ox - c - s exactly": all(v == 2 * ox - c - s for c, v in enumerate(p.cols)),
                "rows land on 2 oy - r - s exactly": all(v == 2 * oy - r - s for r, v in enumerate(p.rows)),
                "something is written": bool(p.expected.any()),
                "a coordinate of -1/2 is cut to 0": not half or w <= 2 * ox or p.cols[2 * ox] == Fraction(-1, 2)}
    return Problem(f"behind{'_half' if half else ''}_{w}x{h}_L{level}", "behind", w, h, ox, oy,
                   (s / F, s / F, -2), dz, level, reached=reached)


def z_zero(w, h, level=0):
    ox, oy = _centre(w, h)
    return Problem(f"z_zero_{w}x{h}_L{level}", "z_zero", w, h, ox, oy, (Fraction(1, 128), Fraction(1, 128), -1), 1.0, level,
                   reached=lambda p: {"Z' is 0": Fraction(p.dz) + Fraction(p.t[2]) == 0,
                                      "nothing is written": not p.expected.any()})


def z_tiny(w, h, level=0):
    """Z' = 2^-40 with half a pixel of translation: every coordinate is (c - ox + 1/2) 2^40 + ox, at least 2^38 in size and so beyond int."""
    ox, oy = _centre(w, h)
    return Problem(f"z_tiny_{w}x{h}_L{level}", "z_tiny", w, h, ox, oy,
                   (Fraction(1, 128), Fraction(1, 128), Fraction(-(2 ** 40 - 1), 2 ** 40)), 1.0, level,
                   reached=lambda p: {"Z' is 2^-40": Fraction(p.dz) + Fraction(p.t[2]) == Fraction(1, 2 ** 40),
                                      "every coordinate is beyond int":
                                          all(abs(v) >= 2 ** 38 for v in p.cols + p.rows),
                                      "nothing is written": not p.expected.any()})


def invalid_1x1():
    return Problem("invalid_1x1", "invalid", 1, 1, 0, 0, (0, 0, 0), 1.0, 0, specials=[(0, 0, 0.0)],
                   reached=lambda p: {"nothing is written": not p.expected.any()})


SHIFTS = [(0.5, 0), (1, 0), (-0.5, 0), (-1, 0), (0, 0.5), (0, 1), (0, -0.5), (0, -1), (0.5, 0.5), (1, 1), (-0.5, -0.5),
          (-1, -1), (0.5, -1), (-1, 0.5)]
SMALL_SHAPES = [(1, 1), (1, 7), (7, 1), (15, 17), (16, 16), (257, 1)]           # (w, h): 1, 7, 7, 255, 256 and 257 pixels
LEVELS = (0, MAX_LEVELS - 1)

_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def small_problems():
    """Every exact problem below the grid-stride size, at level 0 and at the last level."""
    def build():
        out = []
        for level in LEVELS:
            out += [shift(16, 8, sx, sy, level) for sx, sy in SHIFTS]
            out += [shift(16, 8, 0.5, -0.5, level, dz=4.0), shift(16, 8, -1, 1, level, dz=0.125)]
            out += [identity(16, 8, level), halving(32, 16, level), halving(260, 4, level), halving(32, 16, level, dz=0.25),
                    gate(32, 16, level), gate(260, 8, level), inf_depth(32, 16, level), subnormal_depth(32, 16, level),
                    collapse(320, 16, level), behind(32, 16, False, level), behind(31, 16, True, level),
                    behind(32, 16, True, level, dz=2.0), z_zero(16, 8, level), z_tiny(16, 8, level)]
            for w, h in SMALL_SHAPES:
                out += [identity(w, h, level), shift(w, h, 0.5, 0.5, level), shift(w, h, -1, -1, level),
                        shift(w, h, -0.5, 1, level), halving(w, h, level), collapse(w, h, level),
                        behind(w, h, True, level), z_zero(w, h, level)]
        out.append(invalid_1x1())
        names = [p.name for p in out]
        assert len(set(names)) == len(names)
        return out
    return _cached("small", build)


def big_problems():
    """The grid-stride shape: 1024 pixels, the last row bar its first pixel, fall into the second trip of the loop."""
    def build():
        def second_trip(p):
            return {"a winner's source index is in the second trip": int(p.owner.max()) >= GRID_STRIDE}
        out = [identity(BIG_W, BIG_H), collapse(BIG_W, BIG_H), shift(BIG_W, BIG_H, 0.5, 0), shift(BIG_W, BIG_H, -0.5, 1)]
        for p in out:
            p.reached["the image has a second trip"] = BIG_W * BIG_H > GRID_STRIDE >= BIG_W * (BIG_H - 1)
            p.reached.update(second_trip(p))
            p.reached["a second-trip source lands in the expected image"] = bool(
                np.any(p.owner.reshape(-1)[p.owner.reshape(-1) >= 0] >= GRID_STRIDE))
        return out
    return _cached("big", build)


# ------------------------------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------------------------------
SWEEP_DRAWS = 64
SWEEP_SEED = 20260


def _eigen_pose(state):
    """R = Rz(yaw) Ry(pitch) Rx(roll), the reference's eigenPose; only an input here."""
    x, y, z, yaw, pitch, roll = [float(v) for v in state]
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, x],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, y],
                     [-sp, cp * sr, cp * cr, z], [0.0, 0.0, 0.0, 1.0]])


HOLE_VALUES = (0.0, -0.0, -1.0, float("nan"), float("inf"), 2.0 ** -1060)


def sweep_draw(index):
    """Draw `index` of the sweep: dict with gray, depth, rt, K, level, state and the CPU-side counts (`stats`)."""
    def build():
        rs = np.random.RandomState(SWEEP_SEED + index)
        w, h = int(rs.randint(1, 98)), int(rs.randint(1, 98))
        if index % 16 == 5:
            h = 1
        if index % 16 == 13:
            w = 1
        level = int((index * 7 + 3) % MAX_LEVELS)                            # every level four times in 64 draws
        fx = rs.uniform(0.6, 2.0) * max(w, h, 4)
        fy = fx * rs.choice([0.8, 0.93, 1.07, 1.25])
        ox, oy = (w - 1) / 2.0 + rs.uniform(-0.2, 0.2) * w, (h - 1) / 2.0 + rs.uniform(-0.2, 0.2) * h
        if index % 5 == 0:                                                   # a principal point outside the image
            ox, oy = [(-0.3 * w, 0.4 * h), (1.4 * w, 0.5 * h), (0.5 * w, -0.6 * h), (0.5 * w, 1.3 * h + 1)][(index // 5) % 4]
        s = float(2 ** level)
        K = np.array([[fx * s, 0.0, ox * s], [0.0, fy * s, oy * s], [0.0, 0.0, 1.0]])
        gray = rs.randint(1, 256, size=(h, w)).astype(np.uint8)
        depth = rs.uniform(0.5, 4.0, size=(h, w))
        rate = rs.uniform(0.0, 0.3)
        holes = rs.rand(h, w) < rate
        depth[holes] = np.array(HOLE_VALUES)[rs.randint(0, len(HOLE_VALUES), size=int(holes.sum()))]
        # from inter-frame motions to anything; a level meets every angle scale (draws i, i + 16, i + 32, i + 48 share it)
        angles = rs.uniform(-np.pi, np.pi, 3) * [0.01, 0.06, 0.3, 1.0][index // 16]
        if index % 8 < 5:                                                    # mostly in the image plane (yaw turns about z)
            angles[1:] *= 0.1
        state = np.concatenate([rs.uniform(-3, 3, 3) * [0.005, 0.03, 0.15, 1.0][index % 4], angles])
        d = dict(index=index, w=w, h=h, level=level, K=K, gray=gray, depth=depth, state=state, rt=_eigen_pose(state))
        d["stats"] = sweep_stats(d)
        return d
    return _cached(("sweep", index), build)


def sweep_stats(d):
    """Collisions, drops per border and Z' <= 0, counted with a plain numpy projection (coverage accounting only: a source
    within rounding of a border may be counted on the other side; no expectation is derived from this)."""
    h, w = d["gray"].shape
    s = float(2 ** d["level"])
    fx, fy, ox, oy = d["K"][0, 0] / s, d["K"][1, 1] / s, d["K"][0, 2] / s, d["K"][1, 2] / s
    dz = d["depth"]
    ok = dz > 0
    with np.errstate(all="ignore"):
        c, r = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        P = np.stack([(c - ox) * dz / fx, (r - oy) * dz / fy, dz, np.ones_like(dz)])
        T = np.einsum("ab,bhw->ahw", d["rt"][:3], P)
        u, v = T[0] * fx / T[2] + ox, T[1] * fy / T[2] + oy
        fin = ok & np.isfinite(u) & np.isfinite(v) & (np.abs(u) < INT_LIMIT) & (np.abs(v) < INT_LIMIT)
        tu, tv = np.trunc(np.where(fin, u, -9.0)), np.trunc(np.where(fin, v, -9.0))
        inside = fin & (tu >= 0) & (tu < w) & (tv >= 0) & (tv < h)
        flat = (tv * w + tu)[inside].astype(np.int64)
        return dict(collisions=int(flat.size - np.unique(flat).size), landed=int(flat.size),
                    dropped=int(np.count_nonzero(ok & ~inside)),
                    left=int(np.count_nonzero(fin & (tu < 0))), right=int(np.count_nonzero(fin & (tu >= w))),
                    top=int(np.count_nonzero(fin & (tv < 0))), bottom=int(np.count_nonzero(fin & (tv >= h))),
                    behind=int(np.count_nonzero(ok & (T[2] <= 0))), holes=int(np.count_nonzero(~ok)))
