"""CPU checks of the bi-objective and trust-region checkers (tests/biobjective_ref.py, tests/trust_region_ref.py) on the
input classes the randomised sweep (tests/tools/fuzz_objectives.py) draws beyond the seeded tiny cases of
test_biobjective_cpu.py and test_trust_region_cpu.py: NaN, negative and +-inf source depth and depth exactly at either
bound of the depth gate, non-default depth ranges, for the bi-objective zero, negative and beyond-max target depth, and
intrinsics off the half-integer grid.  The vectorised form must equal the literal per-pixel loop to 1e-12 on every one
of them, and the sweep must reach every class.  Then draw_case of fuzz_objectives.py: its FUZZ_ONLY replay draws what
the full sweep draws, and 300 draws per mode reach every size class, geometry, depth defect and range change."""
import os
import sys

import numpy as np
import pytest

import biobjective_ref as bref
import trust_region_ref as tref

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import fuzz_objectives as fo  # noqa: E402

DEFAULT_RANGE = (0.3, 5.0)


def _depth_range(rs):
    """The default range, or one of a few others (bounds that are not short binary fractions among them)."""
    k = int(rs.randint(0, 4))
    if k == 0:
        return DEFAULT_RANGE
    if k == 1:
        return 0.5, 3.0
    return float(rs.uniform(0.4, 1.3)), float(rs.uniform(2.0, 4.0))


def _defect_depth(rs, d, lo, hi):
    """Source depth with holes and, per pixel with some probability, NaN, negative, +-inf, exactly lo, exactly hi and
    beyond hi."""
    h, w = d.shape
    d = d.copy()
    for v, p in ((0.0, 0.1), (np.nan, 0.06), (-1.0, 0.05), (np.inf, 0.03), (-np.inf, 0.03), (lo, 0.08), (hi, 0.08),
                 (hi + 1.5, 0.05)):
        d[rs.uniform(size=(h, w)) < p] = v
    return d


def _intrinsics(rs, w, h):
    """Focal lengths and principal point off the half-integer grid (fx != fy)."""
    fx, fy = rs.uniform(1.0, 6.0), rs.uniform(1.0, 6.0)
    return np.array([[fx, 0, (w - 1) / 2.0 + rs.uniform(-1.3, 1.3)], [0, fy, (h - 1) / 2.0 + rs.uniform(-1.3, 1.3)],
                     [0, 0, 1.0]])


def _state(rs, seed):
    kind = seed % 4
    if kind == 0:
        return np.zeros(6)
    if kind == 1:
        return np.array([0, 0, rs.uniform(-1.5, 3.0), 0, 0, 0])             # zoom: collisions both ways
    if kind == 2:
        return rs.uniform(-0.6, 0.6, 6)
    return rs.normal(0, 0.05, 6)


def _off_grid(K):
    return any(2.0 * v != np.floor(2.0 * v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def _classes(d, lo, hi):
    return dict(nan=np.isnan(d), negative=d < 0, inf=np.isinf(d), at_min=d == lo, at_max=d == hi,
                beyond_max=np.isfinite(d) & (d > hi))


def test_biobjective_vectorised_equals_literal_on_defects_and_ranges():
    seen = dict(intensity_won=0, depth_won_below_n=0, row0_tie=0, jdep_below_n=0, depth_rows_at_n=0,
                nan=0, negative=0, inf=0, at_min=0, at_max=0, beyond_max=0, non_default_range=0, gate_moved=0,
                tgt_zero_read=0, tgt_negative_read=0, tgt_beyond_max_read=0, off_grid=0)
    for seed in range(400):
        rs = np.random.RandomState(10_000 + seed)
        w, h = rs.randint(1, 10), rs.randint(1, 8)
        lo, hi = _depth_range(rs)
        gray = rs.uniform(0, 1, (h, w))
        d0 = _defect_depth(rs, rs.uniform(0.5 * lo, 1.1 * hi, (h, w)), lo, hi)
        i1 = rs.uniform(0, 1, (h, w))
        d1 = rs.uniform(0.5, 4.0, (h, w))
        d1[rs.uniform(size=(h, w)) < 0.1] = 0.0
        d1[rs.uniform(size=(h, w)) < 0.1] = -rs.uniform(0.1, 2.0)
        d1[rs.uniform(size=(h, w)) < 0.1] = hi + rs.uniform(0.5, 3.0)
        gx, gy, dgx, dgy = [rs.normal(0, 1, (h, w)) for _ in range(4)]
        gain = rs.uniform(0.1, 2.0)
        K = _intrinsics(rs, w, h)
        state = _state(rs, seed)
        r, J, nc = bref.literal_system(gray, d0, i1, d1, gx, gy, dgx, dgy, gain, 0, K, state, lo, hi)
        H0, g0 = J.T @ J, J.T @ r
        H, g, st = bref.normal_equations(gray, d0, i1, d1, gx, gy, dgx, dgy, gain, 0, K, state, lo, hi)
        assert st["contributing"] == nc, seed
        assert np.abs(H - H0).max() <= 1e-12 * max(np.abs(H0).max(), 1e-300), seed
        assert np.abs(g - g0).max() <= 1e-12 * max(np.abs(g0).max(), 1e-300), seed
        for k in ("intensity_won", "depth_won_below_n", "row0_tie", "jdep_below_n", "depth_rows_at_n"):
            seen[k] += st[k]
        wp = bref.warp(d0, 0, K, state, lo, hi)
        dv = d0.ravel()
        for k, m in _classes(dv, lo, hi).items():
            assert not np.any(wp["contrib"][m]), (seed, k)                 # every one of them fails the strict gate
            seen[k] += int(m.sum())
        if (lo, hi) != DEFAULT_RANGE:
            seen["non_default_range"] += 1
            wd = bref.warp(d0, 0, K, state, *DEFAULT_RANGE)
            seen["gate_moved"] += int(np.sum(wd["contrib"] != wp["contrib"]))
        t = wp["tgt"][wp["contrib"]]
        seen["tgt_zero_read"] += int(np.sum(d1.ravel()[t] == 0.0))
        seen["tgt_negative_read"] += int(np.sum(d1.ravel()[t] < 0.0))
        seen["tgt_beyond_max_read"] += int(np.sum(d1.ravel()[t] > hi))
        seen["off_grid"] += int(_off_grid(K))
    assert all(v > 0 for v in seen.values()), seen


def test_trust_region_vectorised_equals_literal_on_defects_and_ranges():
    seen = dict(low_edge=0, high_clamp=0, size1=0, collisions=0, out_of_bounds=0, nan=0, negative=0, inf=0, at_min=0,
                at_max=0, beyond_max=0, non_default_range=0, gate_moved=0, off_grid=0)
    for seed in range(400):
        rs = np.random.RandomState(20_000 + seed)
        w, h = rs.randint(1, 10), rs.randint(1, 8)
        lo, hi = _depth_range(rs)
        i0 = rs.uniform(0, 1, (h, w))
        d0 = _defect_depth(rs, rs.uniform(0.5 * lo, 1.1 * hi, (h, w)), lo, hi)
        i1, gx, gy = (rs.normal(0, 1, (h, w)) for _ in range(3))
        K = _intrinsics(rs, w, h)
        state = _state(rs, seed)
        r0, J0, rows0 = tref.literal_rows(i0, d0, i1, gx, gy, 0, K, state, lo, hi)
        ev = tref.evaluate(i0, d0, i1, gx, gy, 0, K, state, lo, hi)
        assert ev["rows"] == rows0, seed
        assert np.abs(ev["r"] - r0).max(initial=0.0) <= 1e-12 * max(np.abs(r0).max(initial=0.0), 1e-300), seed
        assert np.abs(ev["J"] - J0).max(initial=0.0) <= 1e-12 * max(np.abs(J0).max(initial=0.0), 1e-300), seed
        ok, u, v = ev["ok"], ev["u"], ev["v"]
        dv = d0.ravel()
        gate = (lo < dv) & (dv < hi)
        for k, m in _classes(dv, lo, hi).items():
            assert not np.any(ok[m]), (seed, k)
            seen[k] += int(m.sum())
        seen["out_of_bounds"] += int((gate & ~ok).sum())
        seen["collisions"] += int(ok.sum()) - rows0
        if ok.any():
            seen["low_edge"] += int(((u[ok] < 0.5) | (v[ok] < 0.5)).sum())
            seen["high_clamp"] += int(((u[ok] - 0.5 > w - 2) | (v[ok] - 0.5 > h - 2)).sum())
            if w == 1 or h == 1:
                seen["size1"] += int(ok.sum())
        if (lo, hi) != DEFAULT_RANGE:
            seen["non_default_range"] += 1
            evd = tref.evaluate(i0, d0, i1, gx, gy, 0, K, state, *DEFAULT_RANGE)
            seen["gate_moved"] += int(np.sum(evd["ok"] != ok))
        seen["off_grid"] += int(_off_grid(K))
    assert all(v > 0 for v in seen.values()), seen


def test_trust_region_linear_axis_at_its_edges():
    """Truncation toward zero: u in [0, 0.5) keeps taps (0, 1) with a weight of tap 0 above 1 (extrapolation, as the
    reference's LinearInitAxis); u in [W - 0.5, W) clamps both taps to W - 1.  Along rows alike."""
    for c, want in ((0.25, (0, 1, 1.25)), (0.0, (0, 1, 1.5)), (0.75, (0, 1, 0.75)), (7.25, (6, 7, 0.25)),
                    (7.5, (7, 7, 1.0)), (7.75, (7, 7, 1.0))):
        assert tref.linear_axis(c, 8) == want, (c, tref.linear_axis(c, 8))
    assert tref.linear_axis(0.25, 1) == (0, 0, 1.0)


# ---- draw_case of the sweep tool -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", fo.MODES)
@pytest.mark.parametrize("flags", [(), ("big",), ("angles",)], ids=["plain", "big", "angles"])
def test_fuzz_only_replay_draws_what_the_sweep_draws(mode, flags):
    full = fo.draw_cases(40, 5, mode, set(flags))
    for case in (0, 7, 23, 39):
        only = fo.draw_cases(40, 5, mode, set(flags), only={case})
        assert set(only) == {case}
        assert fo.case_key(only[case]) == fo.case_key(full[case]), (mode, flags, case)


@pytest.mark.parametrize("mode", fo.MODES)
def test_draws_reach_every_class(mode):
    cov = fo.coverage(fo.draw_cases(300, 1, mode, set()).values(), mode)
    for k, v in cov.items():
        assert v > 0, (mode, k, cov)
    big = fo.coverage(fo.draw_cases(300, 2, mode, {"big"}).values(), mode)
    assert big["size_big"] > 0 and big["size_strip"] > 0, big
