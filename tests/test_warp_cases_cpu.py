"""tests/warp_cases.py held alone, without a device: its closed-form images against the oracle's warp and, where it is
built, against the reference's own compiled warpImage; the forms the exact problems take on the named shapes, written
out once more as plain slices; and the coverage of the sweep's draws.

Held to the oracle only (the reference's static_cast<int> of a non-finite or out-of-range double is undefined):
warp_cases.NO_REFERENCE_BUILD -- the +inf depth, Z' = 0 and Z' = 2^-40 problems.
"""
import numpy as np

import warp_cases as wc

import phovo_amd  # noqa: F401
from oracle import oracle, reference_build as refb

HAVE_REFERENCE_BUILD = refb.tree_present() or refb.available()


def _held_to_both(p):
    assert all(p.reached.values()), (p.name, [k for k, v in p.reached.items() if not v])
    got = oracle.warp_image(p.gray, p.depth, p.rt, p.K, p.level)
    assert np.array_equal(got, p.expected), (p.name, np.argwhere(got != p.expected)[:8])
    if HAVE_REFERENCE_BUILD and p.reference_build_defined:
        ref = refb.warp_image(p.gray, p.depth, p.rt, p.K, p.level)
        assert np.array_equal(ref, p.expected), (p.name, np.argwhere(ref != p.expected)[:8])
        return 1
    return 0


def test_small_closed_forms_equal_the_oracle_and_the_reference_build():
    held = sum(_held_to_both(p) for p in wc.small_problems())
    left_out = [p.name for p in wc.small_problems() if not p.reference_build_defined]
    assert left_out and all(any(k in n for k in wc.NO_REFERENCE_BUILD) for n in left_out)
    print(f"{len(wc.small_problems())} problems, {held} of them also against the reference build; oracle only: "
          f"{sorted(set(n.rsplit('_', 2)[0] for n in left_out))}")
    if HAVE_REFERENCE_BUILD:
        assert held == len(wc.small_problems()) - len(left_out)


def test_grid_stride_closed_forms_equal_the_oracle_and_the_reference_build():
    for p in wc.big_problems():
        assert p.w * p.h > wc.GRID_STRIDE and int(p.owner.max()) >= wc.GRID_STRIDE
        _held_to_both(p)


def test_every_kind_of_problem_and_every_small_shape_is_there():
    ps = wc.small_problems()
    assert {p.kind for p in ps} >= {"identity", "shift", "halving", "gate", "inf_depth", "subnormal_depth", "collapse",
                                    "behind", "z_zero", "z_tiny", "invalid"}
    assert {p.level for p in ps} == {0, wc.MAX_LEVELS - 1}
    assert {p.w * p.h for p in ps} >= {1, 7, 255, 256, 257}
    assert {(p.w, p.h) for p in ps} >= {(1, 1), (1, 7), (7, 1), (15, 17), (16, 16), (257, 1)}
    assert max(p.w * p.h for p in ps) <= 100 * 100
    assert any(p.kind == "halving" and p.w > 256 for p in ps)              # the sources of a target in different workgroups


def _problem(name):
    return next(p for p in wc.small_problems() if p.name == name)


def test_shifts_written_as_slices():
    """The 16x8 shifts as the slices they are, independent of warp_cases.place."""
    g = wc.gray_ramp(16, 8)
    z = np.zeros_like(g)

    def cols(a, b, c, d):
        e = z.copy()
        e[:, a:b] = g[:, c:d]
        return e
    e = cols(0, 15, 1, 16)                                        # +1/2: columns 0 and 1 on column 0, 1 wins; the last is empty
    assert np.array_equal(_problem("shift_+0.5_+0_16x8_L0").expected, e) and np.all(e[:, 15] == 0) and e[0, 0] == g[0, 1]
    assert np.array_equal(_problem("shift_+1_+0_16x8_L0").expected, e)                  # +1: column 0 on -1.0, dropped
    assert np.array_equal(_problem("shift_-0.5_+0_16x8_L0").expected, g)                # w - 1/2 is cut to w - 1: unchanged
    assert np.array_equal(_problem("shift_-1_+0_16x8_L0").expected, cols(1, 16, 0, 15))  # the last column dropped, 0 empty
    e = z.copy()
    e[0:7] = g[1:8]
    assert np.array_equal(_problem("shift_+0_+0.5_16x8_L0").expected, e)
    assert np.array_equal(_problem("shift_+0_+1_16x8_L0").expected, e)
    assert np.array_equal(_problem("shift_+0_-0.5_16x8_L0").expected, g)
    e = z.copy()
    e[1:8] = g[0:7]
    assert np.array_equal(_problem("shift_+0_-1_16x8_L0").expected, e)
    e = z.copy()
    e[0:7, 0:15] = g[1:8, 1:16]
    assert np.array_equal(_problem("shift_+0.5_+0.5_16x8_L0").expected, e)
    assert np.array_equal(_problem("shift_+1_+1_16x8_L0").expected, e)
    e = z.copy()
    e[1:8, 1:16] = g[0:7, 0:15]
    assert np.array_equal(_problem("shift_-1_-1_16x8_L0").expected, e)
    for level in wc.LEVELS:                                        # K carries 2^level: the answer is level 0's
        assert np.array_equal(_problem(f"shift_+0.5_+0.5_16x8_L{level}").expected, _problem("shift_+0.5_+0.5_16x8_L0").expected)


def test_halving_collapse_and_reflection_written_out():
    g = wc.gray_ramp(32, 16)
    e = np.zeros_like(g)
    e[4:12, 8:24] = g[1::2, 1::2]
    p = _problem("halving_32x16_L0")
    assert np.array_equal(p.expected, e) and np.count_nonzero(e) == 128 and p.collisions == 3 * 128
    p = _problem("collapse_320x16_L0")
    e = np.zeros((16, 320), dtype=np.uint8)
    g = wc.gray_ramp(320, 16)
    e[7, 159], e[7, 160], e[8, 159], e[8, 160] = g[7, 159], g[7, 319], g[15, 159], g[15, 319]
    assert np.array_equal(p.expected, e)
    assert np.bincount(p.targets.reshape(-1)).max() > 1000 and p.collisions == 320 * 16 - 4
    p = _problem("behind_32x16_L0")                                # column' = 32 - c, row' = 16 - r: column 0 and row 0 fall out
    g = wc.gray_ramp(32, 16)
    e = np.zeros_like(g)
    e[1:, 1:] = g[:0:-1, :0:-1]
    assert np.array_equal(p.expected, e)
    p = _problem("behind_half_32x16_L0_dz2")                       # 31.5 - c: cut to 31 - c, and -1/2 (c = 32) does not exist
    assert np.array_equal(p.expected, g[::-1, ::-1])
    p = _problem("behind_half_31x16_L0")                           # ox = 15: 29.5 - c; c = 30 gives -1/2, cut to 0: wins over c = 29
    assert p.cols[30] == -0.5 and p.owner[0, 0] % 31 == 30
    p = _problem("gate_32x16_L0")
    q = _problem("halving_32x16_L0")
    assert p.expected[9, 18] == 0 and q.expected[9, 18] != 0
    assert np.count_nonzero(p.expected != q.expected) == 1


def test_sweep_coverage():
    draws = [wc.sweep_draw(i) for i in range(wc.SWEEP_DRAWS)]
    st = [d["stats"] for d in draws]
    assert len(draws) == 64
    assert all(1 <= d["w"] <= 97 and 1 <= d["h"] <= 97 and d["K"][0, 0] != d["K"][1, 1] for d in draws)
    count = lambda key: sum(s[key] > 0 for s in st)      # noqa: E731
    summary = {k: count(k) for k in ("collisions", "left", "right", "top", "bottom", "behind", "holes", "landed")}
    print(summary)
    assert summary["collisions"] >= 16
    assert min(summary[k] for k in ("left", "right", "top", "bottom")) >= 16
    assert summary["behind"] >= 8
    # a quarter of the draws translates by up to 3 m at depths of 0.5 to 4 m and another few turn out of view: those may
    # clear the image.  The rest, five in eight at the least, must compare images and not zeros.
    assert summary["landed"] >= 40
    assert {d["level"] for d in draws} == set(range(wc.MAX_LEVELS))
    assert any(d["h"] == 1 and d["w"] > 1 for d in draws) and any(d["w"] == 1 and d["h"] > 1 for d in draws)
    out = lambda d: not (0 <= d["K"][0, 2] / 2 ** d["level"] < d["w"] and 0 <= d["K"][1, 2] / 2 ** d["level"] < d["h"])  # noqa: E731
    assert 4 <= sum(out(d) for d in draws) <= 32
    rates = [s["holes"] / (d["w"] * d["h"]) for s, d in zip(st, draws)]
    assert min(rates) == 0.0 or min(rates) < 0.02
    assert max(rates) > 0.2 and max(r for r, d in zip(rates, draws) if d["w"] * d["h"] >= 100) <= 0.45
    kinds = np.concatenate([d["depth"].reshape(-1) for d in draws])
    assert np.isnan(kinds).any() and np.isposinf(kinds).any() and (kinds == 2.0 ** -1060).any() and (kinds < 0).any()
    assert (np.signbit(kinds) & (kinds == 0)).any() and ((kinds == 0) & ~np.signbit(kinds)).any()
    big = [np.abs(d["state"][3:]).max() for d in draws]
    assert max(big) > 2.0 and min(big) < 0.06

