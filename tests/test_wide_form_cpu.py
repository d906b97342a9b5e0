"""CPU pre-checks of tests/wide_form.py: every builder of tests/test_gpu_wide_form.py does, on the oracle alone, what that
module relies on, so that no GPU test can pass for want of a case.  No GPU.

The tiling and the host's look schedule are restated from csrc/gn_wide_kernels.hip and held to its text.  Every size of
the tile table has the tile count and the last-tile pixel count the table names, and losing its last tile changes the
oracle's valid pixels (and, from one chunk on, its pose).  The searched initial states keep every gradient norm 1e-6 from
the threshold, and each batch contains the stop counts that make the host loop end the way its name says.  Every finite
reference is well-posed for its bar: one ulp of fx moves it by less than a quarter of the bar and changes no count.
"""
import os
import re

import numpy as np
import pytest

import extension_forms as ef
import wide_form as wf

import phovo_amd  # noqa: F401
from phovo_amd import native, se3
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _well_posed(ref, what):
    """Finite, and one ulp of fx moves the oracle by less than a quarter of the bar and changes no iteration count."""
    assert ref.finite, what
    moved, its = ref.nudged()
    assert moved < 0.25 * ref.bar and its == ref.its, (what, moved, ref.bar, its, ref.its)


def test_the_restated_constants_are_the_kernel_files():
    src = open(os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc", "gn_wide_kernels.hip")).read()
    assert re.search(r"constexpr int WT = (\d+);", src).group(1) == "256"
    assert re.search(r"constexpr int TILE_CHUNKS = (\d+);", src).group(1) == str(wf.TILE_CHUNKS)
    assert re.search(r"constexpr int SOLVE_T = (\d+);", src).group(1) == str(wf.SUM_SUBSETS * 32)
    assert "t += SOLVE_T / NRED" in src and "(it & 1) * 6" in src and "(done_it & 1) * 6" in src
    assert re.search(r"int next_check = (\d+);", src).group(1) == str(wf.FIRST_LOOK)
    assert f"next_check = it + 1 + {wf.LOOK_EVERY};" in src
    assert f"it + 1 >= next_check && a.max_iter - (it + 1) >= {wf.LOOK_RESERVE}" in src
    # the schedule as a formula
    assert wf.host_looks(16, 230.0) == [4, 12] and wf.host_looks(13, 230.0) == [4] and wf.host_looks(7, 230.0) == []
    assert wf.host_looks(8, 230.0) == [4] and wf.host_looks(50, 230.0) == [4, 12, 20, 28, 36, 44]
    assert wf.host_looks(50, 0.0) == []
    assert wf.launched_iterations(50, 230.0, [1, 3, 2]) == 4 and wf.launched_iterations(50, 230.0, [1, 4, 2]) == 12
    assert wf.launched_iterations(50, 230.0, [11, 4]) == 12 and wf.launched_iterations(50, 230.0, [12, 4]) == 20
    assert wf.launched_iterations(16, 230.0, [11, 4]) == 12 and wf.launched_iterations(16, 230.0, [16, 1]) == 16


# ------------------------------------------------------------------------------------------------------------------------
# 1. tiles
# ------------------------------------------------------------------------------------------------------------------------
def test_the_tile_table_covers_the_interleaved_sum():
    got = {s: (wf.tiles(s[0] * s[1]), wf.last_tile(s[0] * s[1])[1]) for s in wf.TILE_SIZES}
    assert got == wf.TILE_SIZES
    counts = sorted({t for t, _ in got.values()})
    assert counts == [1, 2, 7, 8, 9, 16, 17]                  # below, at and above one and two rounds of the 8 subsets
    assert wf.subset_sizes(112 * 64) == [1] * 7 + [0] and wf.subset_sizes(128 * 64) == [1] * 8
    assert wf.subset_sizes(82 * 100) == [2] + [1] * 7 and wf.subset_sizes(145 * 113) == [3] + [2] * 7
    assert sorted({n for _, n in got.values()}) == [1, 8, 1023, 1024]
    assert all(w * h <= 164 * 200 for w, h in wf.TILE_SIZES)


@pytest.mark.parametrize("size", list(wf.TILE_SIZES), ids=wf.size_id)
def test_the_last_tile_counts(size):
    """Every pixel of the last tile has valid source depth; without the tile the oracle's last iteration counts fewer valid
    pixels -- by the whole tile's in-image pixels -- and, where the tile holds at least a chunk, its pose moves by more than
    1e-6.  A 1- or 8-pixel tile ends in the image's corner, whose Scharr gradient is exactly 0 under reflect-101: there the
    exact count is the check, and the GPU test asserts it exactly."""
    w, h = size
    first, count = wf.last_tile(w * h)
    for i, p in enumerate(wf.tile_pairs(size)):
        tail = p["depth0"].reshape(-1)[first:]
        assert tail.size == count and np.all((tail > wf.MIN_DEPTH) & (tail < wf.MAX_DEPTH)), (size, i)
        ref, dropped = wf.tile_ref(size, i), wf.tile_ref(size, i, dropped=True)
        assert ref.its == [wf.TILE_ITERS] and dropped.its == ref.its
        lost = ref.valid[0] - dropped.valid[0]
        assert lost >= 1, (size, i, lost)               # (the two runs part ways after the first step: not always == count)
        if count >= wf.WAVE:
            assert lost >= count - 2 * w, (size, i, lost)                     # all but what the motion carries out of the image
            if wf.tiles(w * h) == 1:                                          # the only tile: nothing is left to solve with
                assert not dropped.finite and dropped.valid == [0]
            else:
                moved = se3.state_distance(ref.state, dropped.state)
                assert moved > wf.TILE_POSE_MOVES, (size, i, moved)
        assert ref.cond <= wf.COND_MAX and ref.bar == wf.POSE_TOL, (size, i, ref.cond)
        assert ref.flags == 0
        _well_posed(ref, (size, i))


# ------------------------------------------------------------------------------------------------------------------------
# 2. stops
# ------------------------------------------------------------------------------------------------------------------------
def test_the_candidates_keep_their_distance_from_the_threshold():
    cands = wf.candidates()
    assert len(cands) >= 300
    for init, g in cands:
        assert len(g) == wf.LONG and min(abs(x - wf.THRESHOLD) for x in g) >= wf.MARGIN * wf.THRESHOLD
    for max_iter, upto in ((16, 16), (13, 13)):
        assert {wf.stop_count(g, max_iter) for _, g in cands} == set(range(1, upto + 1))
    # the restated stop rule is the oracle's
    for init, g in cands[:40]:
        for max_iter in (16, 13, 7):
            assert wf.stop_ref(init, (max_iter,), (wf.THRESHOLD,)).its == [wf.stop_count(g, max_iter)]


def _batch_facts(name):
    max_iter, thr, states = wf.stop_batches()[name]
    refs = wf.batch_refs(name)
    assert len(set(states)) == len(states)
    for k, r in enumerate(refs):
        assert wf.margin(r, (thr,)) >= wf.MARGIN, (name, k)
        assert r.flags == 0 and r.valid[0] > 1000
        _well_posed(r, (name, k))
    return max_iter, thr, [r.its[0] for r in refs], refs


def test_the_mixed_batch_stops_everywhere():
    assert tuple(wf.stop_batches()) == wf.STOP_BATCHES
    max_iter, thr, stops, refs = _batch_facts("mixed16")
    assert len(stops) == 32 and set(stops) == set(range(1, 17))
    assert {3, 4, 5, 11, 12, 13} <= set(stops)                     # the two looks and their neighbours
    never = [r for r in refs if r.its[0] == 16 and min(r.level_gnorms(0)) >= thr]
    assert len(never) >= 1
    assert any(r.its[0] == 16 and r.gnorm < thr for r in refs)      # and one that meets it in the very last iteration
    assert wf.host_looks(max_iter, thr) == [4, 12] and wf.launched_iterations(max_iter, thr, stops) == 16
    # both slots of the state buffer hold a final state
    assert {s % 2 for s in stops} == {0, 1}
    # the positions are mixed: neighbours differ
    assert sum(a != b for a, b in zip(stops, stops[1:])) >= 24


def test_the_mixed_batch_under_the_other_limits():
    max_iter, thr, stops, _ = _batch_facts("mixed13")
    assert set(stops) == set(range(1, 14)) and stops.count(13) >= 7 and max_iter % 2 == 1
    assert wf.host_looks(max_iter, thr) == [4]
    max_iter, thr, stops, _ = _batch_facts("never_looks7")
    assert wf.host_looks(max_iter, thr) == [] and set(stops) == set(range(1, 8))
    max_iter, thr, stops, _ = _batch_facts("one_look8")
    assert wf.host_looks(max_iter, thr) == [4] and set(stops) == set(range(1, 9))
    assert wf.launched_iterations(max_iter, thr, stops) == 8
    max_iter, thr, stops, _ = _batch_facts("no_threshold5")
    assert thr == 0.0 and stops == [5] * 32 and wf.host_looks(max_iter, thr) == []


def test_the_early_leaving_batches_leave_where_they_say():
    max_iter, thr, stops, _ = _batch_facts("leaves_first_look")
    assert max_iter == wf.LONG and len(stops) == 8 and max(stops) == 3 and min(stops) == 1
    assert wf.launched_iterations(max_iter, thr, stops) == 4
    max_iter, thr, stops, _ = _batch_facts("leaves_second_look")
    assert max_iter == wf.LONG and len(stops) == 8 and max(stops) == 11 and min(stops) == 1
    assert sum(5 <= s <= 11 for s in stops) >= 2 and any(s <= 3 for s in stops)
    assert wf.launched_iterations(max_iter, thr, stops) == 12
    # the pair set enqueued behind them on the same engine is another one
    for name in wf.EARLY_LEAVING:
        assert not set(wf.stop_batches()[name][2]) & set(wf.mixed_states()[:8])


def test_two_levels_enter_level_zero_from_either_slot():
    w, h = wf.TWO_SIZE
    assert oracle.level_size(w, h, 1) == wf.STOP_SIZE
    assert (wf.tiles(w * h), wf.last_tile(w * h)[1]) == (33, 32) and wf.tiles(82 * 100) == 9
    refs = wf.two_level_refs()
    assert len(refs) == 8 and len(set(wf.two_level_states())) == 8
    level1 = [r.its[1] for r in refs]
    assert sum(c % 2 for c in level1) == 4, level1
    assert len(set(level1)) >= 3 and len({r.its[0] for r in refs}) >= 3, [r.its for r in refs]
    for k, r in enumerate(refs):
        assert wf.margin(r, wf.TWO_MIN_GRAD) >= wf.MARGIN and r.flags == 0
        _well_posed(r, ("two levels", k))
    # some leave a level through its threshold, some through max_iter
    assert any(r.its[1] < wf.TWO_MAX_ITER[1] for r in refs) and any(r.its[0] < wf.TWO_MAX_ITER[0] for r in refs)


# ------------------------------------------------------------------------------------------------------------------------
# 3. position and batch size
# ------------------------------------------------------------------------------------------------------------------------
def test_the_forty_pair_batch_extends_the_mixed_one():
    s32, s40 = wf.mixed_states(32), wf.mixed_states(40)
    assert s40[:32] == s32 and len(set(s40)) == 40 and wf.POSITION_SIZES == (32, 40)
    for k, s in enumerate(s40[32:]):
        r = wf.stop_ref(s, (16,), (wf.THRESHOLD,))
        assert wf.margin(r, (wf.THRESHOLD,)) >= wf.MARGIN
        _well_posed(r, ("forty", k))


# ------------------------------------------------------------------------------------------------------------------------
# 4. no rows, few rows
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wf.NO_ROWS))
def test_the_pair_without_rows_fails_in_its_first_solve(name):
    size, max_iter = wf.NO_ROWS[name]
    nl = len(max_iter)
    bad = wf.no_rows_ref(name, wf.BAD_SLOT)
    assert not bad.finite and bad.valid == [0] * nl
    assert bad.first_nonfinite == [1] * nl, bad.first_nonfinite          # no row: the first solve of every level already fails
    for k in range(8):
        if k != wf.BAD_SLOT:
            r = wf.no_rows_ref(name, k)
            assert r.its == list(max_iter) and r.flags == 0
            _well_posed(r, (name, k))


@pytest.mark.parametrize("n_valid", wf.FEW_ROWS)
def test_the_few_valid_depths_are_spread_over_the_tiles(n_valid):
    w, h = wf.STOP_SIZE
    px = wf.few_rows_pixels(n_valid)
    first, count = wf.last_tile(w * h)
    assert len(set(px)) == n_valid and sum(k >= first for k in px) == 1
    in_tiles = {k // wf.TILE_PX for k in px}
    assert len(in_tiles) == min(n_valid, wf.tiles(w * h)), in_tiles
    d = wf.few_rows_pair(n_valid)["depth0"].reshape(-1)
    assert int(np.sum((d > wf.MIN_DEPTH) & (d < wf.MAX_DEPTH))) == n_valid and np.count_nonzero(d) == n_valid
    ref = wf.few_rows_ref(n_valid)
    assert ref.trace[0]["valid_pixels"] == n_valid              # from the zero state every one of them lands on itself
    if n_valid >= 40:
        assert not wf.wild(ref.state) and ref.its == [wf.FEW_ITERS] and ref.valid[0] >= 6


# ------------------------------------------------------------------------------------------------------------------------
# 5. half pixels
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("size", wf.HALF_SIZES, ids=wf.size_id)
def test_every_projection_is_an_exact_half(size, sign):
    w, h = size
    tc, tr = wf.half_pixel_targets(size, sign)
    cc, rr = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    assert np.array_equal(tc, cc + 0.5 * sign) and np.array_equal(tr, rr + 0.5 * sign)
    _, _, state, ref = wf.half_pixel(size, sign)
    assert ref.its == [1] and ref.finite and np.linalg.norm(ref.state - state) > 1e-6
    # half away from zero: +0.5 loses the last row and column, -0.5 the first (round(-0.5) = -1)
    assert ref.valid == [(w - 1) * (h - 1)]
    assert ref.bar == wf.POSE_TOL and ref.flags == 0
    assert wf.tiles(w * h) in (3, 9)


# ------------------------------------------------------------------------------------------------------------------------
# 6. strips
# ------------------------------------------------------------------------------------------------------------------------
def test_enough_strips_are_finite_and_the_others_can_be_followed():
    _, ocfg = ef.configs([wf.STRIP_ITERS])
    cases = finite = 0
    for size in ef.STRIPS:
        p, states, planes = wf.strip_case(size)
        assert len(states) == 3
        for k, init in enumerate(states):
            e = ef.expect(ocfg, p["K"], planes, init)           # (asserts the one-ulp guard where the oracle is finite)
            cases += 1
            finite += e.finite
            if not e.finite:
                assert wf.strip_trace_loses_state(ocfg, p["K"], planes, init), (size, k)
    assert cases == 18 and finite >= wf.STRIP_MIN_FINITE, (cases, finite)
