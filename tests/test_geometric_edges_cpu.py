"""CPU pre-checks of the inputs of tests/test_gpu_geometric_edges.py (tests/geometric_edges.py), with the checkers alone
(tests/geometric_ref.py, tests/geometric_system_ref.py) on pyramids built by the oracle's producers: every fixture the GPU file
compares keeps the three margins of test_gpu_geometric._compare (gradient threshold and residual gate 1e-6 relative, pixel
centres CELL_FLOOR), every fixture it holds to the flat bar has cond(H) <= 1e5, the exact positions give the closed-form row
counts and the clamp bands and tap-gate branches they were built for, the large-angle starts leave a flat state per axis,
sign and branch, and the committed seeds of the rank-test problems are the ones the search finds.  No GPU."""
import numpy as np
import pytest

import affine_edges as ae
import edge_states
import geometric_cases as gc
import geometric_edges as ge
import geometric_ref as gr
import geometric_system_ref as gsr


def _margins(ref, what):
    assert ref["margin"] > ge.MARGIN_FLOOR, (what, ref["margin"])
    assert ref["gate_margin"] > ge.MARGIN_FLOOR, (what, ref["gate_margin"])
    assert ref["cell_margin"] > gc.CELL_FLOOR, (what, ref["cell_margin"])


def _holds(ref, what):
    """A fixture held to the flat bar: finite, cond(H) <= 1e5, the three margins."""
    assert np.all(np.isfinite(ref["state"])), what
    assert ref["cond"] <= 1e5 and ge.flat(ref), (what, ref["cond"])
    _margins(ref, what)


def _block_margins(b, what):
    assert b["cell_margin"] > gc.CELL_FLOOR and b["gate_margin"] > gsr.MARGIN_FLOOR, (what, b["cell_margin"], b["gate_margin"])


# ---- A. exact positions --------------------------------------------------------------------------------------------
# (w, h, range) -> depth rows per shift, from rows_loop (24x20) and the checker's level loop, which agree below
EXACT_DEPTH_ROWS = {
    (24, 20, (0.3, 5.0)): {0.25: 345, -0.25: 343, 0.5: 314, -0.5: 314, 0.75: 312, -0.75: 312},
    (24, 20, (0.5, 2.0)): {0.25: 242, -0.25: 257, 0.5: 215, -0.5: 232, 0.75: 214, -0.75: 231},
    (75, 53, (0.3, 5.0)): {0.25: 3556, -0.25: 3549, 0.5: 3465, -0.5: 3466},
    (75, 53, (0.5, 2.0)): {0.25: 3206, -0.25: 3195, 0.5: 3115, -0.5: 3116},
}


def test_the_exact_limit_lies_off_the_residual_grid():
    """D1(u, v) - Z' is a multiple of 1/1024 in part A: the limit is none, and stays 1e-4 relative away from all of them."""
    k = ge.EXACT_LIMIT * 1024.0
    assert abs(k - round(k)) / k > 1e-4 and (ge.EXACT_LIMIT * 256.0) % 1.0 != 0.0


@pytest.mark.parametrize("depth_range", ge.RANGES, ids=["default_range", "range_0.5_2"])
@pytest.mark.parametrize("w,h", list(ge.EXACT_SIZES), ids=["24x20", "75x53"])
def test_exact_positions_rows_bands_and_conditioning(w, h, depth_range):
    for shift in ge.EXACT_SIZES[(w, h)]:
        K, planes, state = ge.exact_problem(w, h, shift, depth_range)
        expected = ae.exact_rows(planes[1], shift)
        assert expected == ae.exact_rows(ae.exact_problem(w, h, shift, depth_range)[1][1], shift)      # the affine file's count
        ref = gr.optimize([planes], K, ge.exact_cfg(depth_range), state)
        assert ref["valid_pixels"] == [expected] and ref["iterations"] == [1] and ref["flags"] == 0
        assert ref["depth_rows"] == [EXACT_DEPTH_ROWS[(w, h, depth_range)][shift]], (shift, ref["depth_rows"])
        _holds(ref, (w, h, shift, depth_range))
        assert ref["cond"] < (3e4 if w == 24 else 1e3), ref["cond"]         # 24x20: 1.9e4 ... 2.5e4; 75x53: 5.1e2 ... 5.8e2
        b = gsr.blocks(planes, 0, K, state, ge.EXACT_SIGMA, ge.EXACT_LIMIT, *depth_range)
        _block_margins(b, (w, h, shift))
        assert (b["rows"], b["depth_rows"]) == (expected, ref["depth_rows"][0])
        # the gate off (the GPU file runs both): more depth rows, the same margins and flatness
        off = gr.optimize([planes], K, dict(ge.exact_cfg(depth_range), max_depth_residual=[0.0]), state)
        _holds(off, (w, h, shift, depth_range, "gate off"))
        assert off["valid_pixels"] == [expected] and off["depth_rows"][0] > ref["depth_rows"][0] and off["flags"] == 0
        if (w, h) != (24, 20):
            continue
        loop = gr.rows_loop(planes, 0, K, state, ge.EXACT_SIGMA, ge.EXACT_LIMIT, *depth_range)
        st = loop["stats"]
        assert int(loop["rows"].sum()) == expected and int(loop["drows"].sum()) == ref["depth_rows"][0]
        assert st["gate"] == int(np.sum(planes[1] != 1.0)) and st["oob"] == w * h - st["gate"] - expected
        seen = {k for k in ("c-", "c+", "r-", "r+") if st[k] > 0}
        assert seen == ae.exact_bands(shift), (shift, seen)
        if abs(shift) == 0.25:
            assert st["zero_dgx"] > 0 and st["zero_dgy"] > 0 and st["oob"] == 0
        else:
            assert st["zero_dgx"] == 0 and st["zero_dgy"] == 0 and st["oob"] > 0
        assert min(st["tap_low"], st["tap_high"], st["tap_nan"], st["residual_gate"]) > 0, st


@pytest.mark.parametrize("w,h", list(ge.EXACT_SIZES), ids=["24x20", "75x53"])
def test_the_second_range_changes_both_row_counts(w, h):
    """The marks at 0.4 and 3.0 pass 0.3 / 5.0 and fail 0.5 / 2.0, in the source and in the target depth: a kernel that took
    a bound from a constant, or the taps' bounds from somewhere else, reports the other range's counts."""
    for shift in ge.EXACT_SIZES[(w, h)]:
        counts = []
        for depth_range in ge.RANGES:
            K, planes, state = ge.exact_problem(w, h, shift, depth_range)
            b = gsr.blocks(planes, 0, K, state, ge.EXACT_SIGMA, ge.EXACT_LIMIT, *depth_range)
            if depth_range != ge.RANGES[0]:
                # these planes under the default range: both counts differ, so a kernel with 0.3 / 5.0 built in shows
                o = gsr.blocks(planes, 0, K, state, ge.EXACT_SIGMA, ge.EXACT_LIMIT, *ge.RANGES[0])
                assert o["rows"] > b["rows"] and o["depth_rows"] > b["depth_rows"], (shift, depth_range)
            counts.append((b["rows"], b["depth_rows"]))
        assert counts[0][0] > counts[1][0] and counts[0][1] > counts[1][1], (shift, counts)
    # ... and the source's bounds are not the taps': with the marks in the target depth alone removed, only depth rows return
    K, planes, state = ge.exact_problem(w, h, 0.25, ge.RANGES[1])
    d1 = planes[5].copy()
    d1[(d1 == 0.4) | (d1 == 3.0)] = 1.0
    a = gsr.blocks(planes, 0, K, state, ge.EXACT_SIGMA, ge.EXACT_LIMIT, *ge.RANGES[1])
    b = gsr.blocks(planes[:5] + (d1,), 0, K, state, ge.EXACT_SIGMA, ge.EXACT_LIMIT, *ge.RANGES[1])
    assert b["rows"] == a["rows"] and b["depth_rows"] > a["depth_rows"]


# ---- B. large angles -----------------------------------------------------------------------------------------------
def test_large_angle_starts_leave_a_flat_pair_per_axis_sign_and_branch():
    """Of the 32 starts on the 80x60 scene of seed 66: 25 finite with cond <= 1e5 (the flat bar; the largest is 3.6e4), none
    finite with a larger cond, 7 that lose every row and go non-finite; every (axis, sign, branch) keeps a flat state with
    more than 100 rows on both levels."""
    p = ge.angle_pair()
    pyr = ge.pyramid(p, 2)
    classes, good = dict(flat=0, conditioned=0, nonfinite=0), set()
    for s in edge_states.initial_states():
        ref = gr.optimize(pyr, p["K"], ge.angle_cfg(), s)
        kind = ge.angle_class(ref)
        classes[kind] += 1
        _margins(ref, s)
        if kind == "nonfinite":
            assert ref["flags"] & gr.PAIR_NONFINITE
        elif kind == "flat":
            assert ge.flat(ref)
            if min(ref["valid_pixels"]) > 100:
                good.add(ae.angle_label(s))
    print(classes)
    assert sum(classes.values()) == 32
    assert good == ge.ALL_LABELS, ge.ALL_LABELS - good
    assert classes == ge.ANGLE_CLASSES, classes


def test_evaluate_states_of_the_large_angle_batch_keep_their_margins():
    p = ge.angle_pair()
    pyr = ge.pyramid(p, 2)
    empty = 0
    for i, s in enumerate(edge_states.initial_states()):
        for level in (0, 1):
            for limit in ge.ANGLE_EVAL_LIMITS:
                b = gsr.blocks(pyr[level], level, p["K"], s, ge.ANGLE_SIGMA, limit)
                _block_margins(b, (i, level, limit))
                empty += b["rows"] == 0
    assert empty == 4 * 4                                      # pitch +-1.2 and the two starts at pi - 0.3: no row on either level


def test_large_motions_and_nonfinite_starts():
    for p, init in ae.motion_pairs():
        ref = gr.optimize(ge.pyramid(p, 1), p["K"], ge.motion_cfg(), init)
        _holds(ref, p["motion"][3])
        assert ref["iterations"][0] < ge.MOTION_MAX_ITER[0] and abs(ref["state"][3] - p["motion"][3]) < 0.05
        assert ref["depth_rows"][0] > 10000
    p = ge.angle_pair()
    pyr = ge.pyramid(p, 2)
    states, bad = ae.nonfinite_batch()
    for k, s in enumerate(states):
        ref = gr.optimize(pyr, p["K"], ge.angle_cfg(), s)
        if k in bad:
            assert ref["iterations"] == [1, 1] and ref["valid_pixels"] == [0, 0] and ref["depth_rows"] == [0, 0]
            assert ref["flags"] == gr.PAIR_RANK_DEFICIENT | gr.PAIR_NONFINITE
        else:
            _holds(ref, k)
            assert ref["flags"] == 0


# ---- C. work queue -----------------------------------------------------------------------------------------------------
def test_work_queue_combinations_hold_the_flat_bar():
    K, frames = ge.work_queue_frames()
    states, pick, which = ge.work_queue_draw()
    assert np.all(states != 0.0) and set(pick.tolist()) == set(range(6)) and set(which.tolist()) == {0, 1, 2, 3}
    assert len({(int(a), int(b)) for a, b in zip(which, pick)}) == 24          # every (pair, state) combination is drawn
    finals = set()
    for kind in range(len(ge.WQ_KINDS)):
        pyr = ge.pyramid(ge.work_queue_pair(frames, kind), ge.WQ_LEVELS)
        assert [lv[0].size for lv in pyr] == [480, 120]
        for b in range(len(states)):
            ref = gr.optimize(pyr, K, ge.work_queue_cfg(), states[b])
            if kind == 2:                                     # an all-NaN source depth
                assert ref["valid_pixels"] == [0, 0] and ref["flags"] == gr.PAIR_RANK_DEFICIENT | gr.PAIR_NONFINITE
                continue
            _holds(ref, (kind, b))
            assert ref["flags"] == 0 and ref["iterations"] == ge.WQ_MAX_ITER
            assert (ref["depth_rows"] == [0, 0]) == (kind == 1)
            finals.add(ref["state"].tobytes())
    assert len(finals) == 18                                  # a start state that leaked from another pair changes the answer


# ---- D. mixed batch, skipped level -------------------------------------------------------------------------------------
def test_mixed_batch_pairs():
    assert set(ge.MIX_KINDS) == set(ge.MIX_SEEDS) and len(ge.MIX_KINDS) == 12
    for kind, p in ge.mixed_pairs().items():
        ref = gr.optimize(ge.pyramid(p, ge.MIX_LEVELS), p["K"], ge.mixed_cfg(), ge.START)
        if kind == "nan_source":
            assert ref["valid_pixels"] == [0, 0, 0] and ref["iterations"] == [1, 1, 1]
            assert ref["flags"] == gr.PAIR_RANK_DEFICIENT | gr.PAIR_NONFINITE
            continue
        _holds(ref, kind)
        assert ref["flags"] == 0 and min(ref["valid_pixels"]) >= 300
        if kind == "no_target_depth":
            assert ref["depth_rows"] == [0, 0, 0] and ref["depth_cost"] == [0.0, 0.0, 0.0]
        else:
            assert min(ref["depth_rows"]) > 100
    pairs = ge.mixed_pairs()
    holes, whole = (gr.optimize(ge.pyramid(pairs[k], ge.MIX_LEVELS), pairs[k]["K"], ge.mixed_cfg(), ge.START)
                    for k in ("target_holes", "healthy0"))
    assert holes["depth_rows"][0] < 0.6 * whole["depth_rows"][0]      # the holes cost depth rows, not photometric rows


def test_skipped_level_reports_nothing_and_changes_the_result():
    p = ge.skip_pair()
    skip = gr.optimize(ge.pyramid(p, 3, ge.SKIP_MAX_ITER), p["K"], ge.skip_cfg(ge.SKIP_MAX_ITER), ge.START)
    full = gr.optimize(ge.pyramid(p, 3), p["K"], ge.skip_cfg(ge.FULL_MAX_ITER), ge.START)
    for ref in (skip, full):
        _holds(ref, ref["iterations"])
        assert ref["flags"] == 0
    assert skip["iterations"] == [5, 1, 5] and full["iterations"] == [5, 5, 5]
    assert (skip["valid_pixels"][1], skip["depth_rows"][1], skip["photometric_cost"][1], skip["depth_cost"][1]) == (0, 0, 0.0, 0.0)
    assert full["depth_rows"][1] > 1000
    assert np.abs(skip["state"] - full["state"]).max() > 1e3 * gr.pose_bar(full["cond"], full["state"])


# ---- E. row counts around the rank test ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ge.ROWS_LAYOUTS)
def test_rank_test_problem_is_the_best_of_its_seed_range_and_well_posed(layout):
    """The committed seed is the one the search finds (smallest worst cond(H) over 6 and 7 rows, ROWS_ITER iterations).  6
    and 7 rows: flags 0, flat bar.  5 photometric rows: RANK_DEFICIENT -- the flag counts photometric rows only -- yet on
    both committed seeds the 5 depth rows supply the rank: the checker's state is finite with cond(H) <= 1e5, so the GPU
    file holds the state too.  7 rows under a target depth that fails every tap: 7 rows, 0 depth rows, a depth cost of 0."""
    conds = [ge.rows_worst_cond(s, layout) for s in ge.ROWS_SEARCH]
    seed = int(np.argmin(conds))
    assert seed == ge.ROWS_SEED[layout] and conds[seed] <= 1e3, (seed, conds[seed])
    print(layout, seed, conds[seed])
    for count in ge.ROWS_COUNTS:
        K, planes = ge.rows_problem(seed, layout, count)
        chunks = {k // 64 for k in np.flatnonzero(np.isfinite(planes[1]).reshape(-1))}
        if layout == "one_chunk":
            assert len(chunks) == 1
        else:
            assert {c % 4 for c in chunks} == {0, 1, 2, 3}
        for mi in ([1], [ge.ROWS_ITER]):
            ref = gr.optimize([planes], K, ge.rows_cfg(mi), ge.START)
            _holds(ref, (layout, count, mi))
            assert ref["valid_pixels"] == [count] and ref["depth_rows"] == [count] and ref["iterations"] == mi
            assert ref["flags"] == (gr.PAIR_RANK_DEFICIENT if count < 6 else 0)
            assert ref["noise_level"] == (0 if count < 6 else None)
    K, planes = ge.rows_problem(seed, layout, 7, target_depth=False)
    for mi in ([1], [ge.ROWS_ITER]):
        ref = gr.optimize([planes], K, ge.rows_cfg(mi), ge.START)
        _holds(ref, (layout, "no target depth", mi))
        assert ref["valid_pixels"] == [7] and ref["depth_rows"] == [0] and ref["depth_cost"] == [0.0] and ref["flags"] == 0


# ---- F. thresholds at small sizes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ge.THR_SIZES, ids=["24x20", "75x53"])
def test_threshold_fixtures_end_every_level_by_the_threshold(w, h):
    p = ge.threshold_pair(w, h)
    pyr = ge.pyramid(p, 2)
    c = ge.threshold_cfg(w, h)
    ref = gr.optimize(pyr, p["K"], c, ge.START)
    print(w, h, ref["iterations"], ref["margin"], ref["gate_margin"])
    _holds(ref, (w, h))
    assert ref["flags"] == 0 and all(3 <= it <= 8 for it in ref["iterations"]), ref["iterations"]
    assert ref["margin"] > 0.1 and min(ref["depth_rows"]) > 50
    # the depth rows are in the g the threshold tests: without them (sigma -> 0 is not allowed; a target without depth) the
    # iteration counts differ
    q = dict(p, depth1=np.zeros_like(p["depth1"]))
    photo = gr.optimize(ge.pyramid(q, 2), p["K"], c, ge.START)
    assert photo["iterations"] != ref["iterations"], photo["iterations"]
    # ... and lambda and the weights are per level: exchanged, the result is more than a thousand bars away
    bar = gr.pose_bar(ref["cond"], ref["state"])
    for other in (dict(c, lam=c["lam"][::-1]), dict(c, depth_weight=c["depth_weight"][::-1])):
        alt = gr.optimize(pyr, p["K"], other, ge.START)
        assert np.abs(alt["state"] - ref["state"]).max() > 1e3 * bar


# ---- G. tiles and chunks -----------------------------------------------------------------------------------------------
def test_tile_and_chunk_fixtures():
    assert [w * h for w, h in ge.TILE_SIZES] == [1024, 1025, 8192, 8256]
    assert [-(-w * h // 1024) for w, h in ge.TILE_SIZES] == [1, 2, 8, 9]
    for w, h in ge.TILE_SIZES:
        p = ge.tile_pair(w, h)
        planes = ge.pyramid(p, 1)[0]
        for s in ge.tile_states():
            for limit in ge.TILE_LIMITS:
                b = gsr.blocks(planes, 0, p["K"], s, ge.TILE_SIGMA, limit)
                _block_margins(b, (w, h, s[3], limit))
                assert b["rows"] > 500 and b["depth_rows"] > 300
        if w * h > 1024:                                       # the last tile holds rows of both blocks: it is not idle
            tail = np.zeros(w * h, dtype=bool)
            tail[(w * h - 1) // 1024 * 1024:] = True
            v = gr.rows_vectorised(planes, 0, p["K"], ge.START, ge.TILE_SIGMA, 0.0)
            assert (v["drows"] & tail).sum() > 0, (w, h)
    assert [-(-w * h // 64) for w, h in ge.CHUNK_SIZES] == [3, 12]
    for w, h in ge.CHUNK_SIZES:
        p = ge.tile_pair(w, h)
        ref = gr.optimize(ge.pyramid(p, 1), p["K"], ge.cfg(ge.CHUNK_MAX_ITER, weight=ge.CHUNK_SIGMA, limit=ge.CHUNK_LIMIT),
                          ge.START)
        _holds(ref, (w, h))
        assert ref["flags"] == 0 and ref["depth_rows"][0] > 100
