"""CPU pre-checks of the inputs of tests/test_gpu_inverse_robust_edges.py (tests/inverse_robust_edges.py).
A: every placed median has the closed form the GPU file asserts -- against inverse_robust_ref.median_loop and against
inverse_robust_ref.optimize under lambda 0 after 1 and after 3 iterations --, the placements sit where their names say, and
three mutants of the median rule each change what some placement expects.  B and C: objective 5's edge fixtures
(tests/inverse_edges.py) under the robust checker keep the distances that exact counts need (bins, delta, gradient
thresholds), hold the flat pose bar, and at inverse_robust_edges.UNIT_SCALE have no weight but 1 on any iteration and end
where objective 5's checker ends.  No GPU."""
import numpy as np
import pytest

import edge_states
import inverse_edges as ie
import inverse_ref as ir
import inverse_robust_cases as cases
import inverse_robust_edges as re6
import inverse_robust_ref as rr

BOTH = ir.PAIR_RANK_DEFICIENT | ir.PAIR_NONFINITE


# ---- A. placed medians -----------------------------------------------------------------------------------------------------
def _rule(placement, scale, half_of=lambda n: (n + 1) // 2, reached=lambda cum, half: cum >= half,
          beyond=lambda ar, delta: ar > delta):
    """inverse_robust_edges.placed_expect with its three decisions as parameters: (delta, outliers)."""
    placement = sorted(placement)
    half = half_of(sum(c for _, c in placement))
    before = 0
    for k, count in placement:
        if reached(before + count, half):
            break
        before += count
    delta = scale * ((float(k) + float(half - before) / float(count)) * 2.0 ** -12)
    return delta, sum(c for b, c in placement if beyond((b + 0.5) / 4096.0, delta))


def _median_bin(placement):
    placement = sorted(placement)
    half = (sum(c for _, c in placement) + 1) // 2
    cum = 0
    for k, count in placement:
        cum += count
        if cum >= half:
            return k, cum == half


def test_the_placements_sit_where_the_issue_asks():
    where = {name: _median_bin(p) for name, p in re6.PLACED.items()}
    bins = [k for k, _ in where.values()]
    for wave in range(4):
        inside = [k for k in bins if k // 1024 == wave]
        assert {0, 15} <= {k % 16 for k in inside}, wave                    # a thread's first and last bin
        assert {0, 63} <= {(k // 16) % 64 for k in inside}, wave            # the wave's first and last lane
    assert {(k >> 6) & 15 for name, (k, _) in where.items() if name.startswith("swizzle")} == set(range(16))
    for k in (1010, 1030, 2040, 2050, 3060, 3080):
        assert k in bins
    # `half` met exactly at a bin's end: at a thread's last bin inside a wave, at a wave's last bin, with and without a gap
    exact = {name: k for name, (k, met) in where.items() if met}
    assert {exact[f"half at the end of {n}"] for n in ("wave 0", "wave 1", "wave 2")} == {1023, 2047, 3071}
    assert {exact[f"half at the end of {n}"] for n in ("thread 21", "thread 149")} == {351, 2399}
    for n in ("thread 21", "thread 149", "wave 0", "wave 1", "wave 2"):
        assert exact[f"half at the end of {n}, then a gap"] == exact[f"half at the end of {n}"]
    assert all(not met and k == where[name[:-len(", one moved")]][0] + 1 for name, (k, met) in where.items()
               if name.endswith("one moved"))
    # the owning thread has empty bins in front of the median's, and earlier waves hold rows
    assert where["thread 85 j=2 and j=9"][0] % 16 == 9 and where["thread 149 j=2 and j=9 behind wave 0"][0] == 16 * 149 + 9
    assert sorted({k // 1024 for k, _ in re6.PLACED["below: every earlier wave"]}) == [0, 1, 2, 3]
    assert where["below: every earlier wave"][0] // 1024 == 3
    rows = {name: sum(c for _, c in p) for name, p in re6.PLACED.items()}
    assert rows["n = 479"] == 479 and rows["n = 451, wave 2"] == 451 and where["n = 451, wave 2"][0] // 1024 == 2
    assert rows["n = 1"] == 1 and rows["n = 2"] == 2
    assert {where[f"all in bin {k}"][0] // 1024 for k in (300, 1300, 2300, 3300)} == {0, 1, 2, 3}
    assert all(n <= re6.N_PIXELS for n in rows.values())
    assert re6.PLACED["tie"] == [(10, 140), (1500, 200), (3000, 140)]


@pytest.mark.parametrize("name", re6.PLACED_NAMES)
def test_placed_medians_have_their_closed_forms(name):
    placement = re6.PLACED[name]
    planes = re6.placed_planes(name)
    i0, d0, gx0, gy0, i1 = planes
    R, t = ir.eigen_rt(np.zeros(6))
    r, _, rows = ir.rows_vectorised(planes, 0, cases.EDGE_K, R, t)
    np.testing.assert_array_equal(rows, np.isfinite(d0).reshape(-1))
    np.testing.assert_array_equal(r[rows], i1.reshape(-1)[rows])            # exact: the residual is the target's value
    np.testing.assert_array_equal(np.sort(r[rows] * 4096.0), np.sort(np.repeat([k + 0.5 for k, _ in placement],
                                                                               [c for _, c in placement])))
    assert bool(gx0.any()) == (name not in re6.PLACED_NO_GRADIENT)
    for scale in re6.PLACED_SCALES:
        n, delta, outliers = re6.placed_expect(placement, scale)
        assert (delta, outliers) == _rule(placement, scale)
        assert rr.median_loop(r[rows]) * scale == delta and rr.median_vectorised(r[rows]) * scale == delta
        tie = scale == re6.TIE_SCALE and name in re6.PLACED_TIES
        for mi in re6.PLACED_MAX_ITER:
            ref = rr.optimize([planes], cases.EDGE_K, re6.placed_cfg(mi), scale_factor=scale)
            assert ref["valid_pixels"] == [n] and ref["delta"] == [delta] and ref["outliers"] == [outliers], (scale, mi, ref)
            if n >= 6:
                assert np.isfinite(ref["cond"]) and ref["flags"] == 0 and ref["iterations"] == [mi]
                assert not ref["state"].any()                               # -0 * step: the pose never moves
            else:                                                           # H exactly zero: an exact zero pivot
                assert ref["flags"] == BOTH and ref["iterations"] == [1] and np.all(np.isnan(ref["state"]))
            # no |r| near its delta, or exactly on it
            assert (ref["delta_margin"] == 0.0) if tie else (ref["delta_margin"] >= cases.DELTA_MARGIN_FLOOR), (scale, mi)
    if name == "tie":
        assert re6.placed_expect(placement, re6.TIE_SCALE) == (480, 1500.5 / 4096.0, 140)
    if name.startswith("all in bin"):
        assert re6.placed_expect(placement, re6.TIE_SCALE)[1:] == ((placement[0][0] + 0.5) / 4096.0, 0)
    if name == "half at the end of wave 0":
        assert re6.placed_expect(placement, 1.0)[1] == 1024.0 / 4096.0
    if name == "half at the end of wave 0, one moved":
        assert re6.placed_expect(placement, 1.0)[1] == (1024.0 + 1.0 / 241.0) / 4096.0
    assert re6.placed_expect(placement, 0.5)[2] > 0                         # a non-zero closed form


# (mutant, its three decisions, the placement it changes, under which scale factor)
MUTANTS = [
    ("half = n // 2", dict(half_of=lambda n: n // 2), "n = 479", rr.DEFAULT_SCALE),
    ("the first bin whose cumulative count is ABOVE half", dict(reached=lambda cum, half: cum > half),
     "half at the end of wave 0, then a gap", rr.DEFAULT_SCALE),
    ("outliers counted with >=", dict(beyond=lambda ar, delta: ar >= delta), "tie", re6.TIE_SCALE),
]


@pytest.mark.parametrize("what,decisions,caught_by,scale", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_placements_tell_the_median_rule_from_its_mutants(what, decisions, caught_by, scale):
    changed = [name for name, p in re6.PLACED.items() for s in re6.PLACED_SCALES
               if s == scale and _rule(p, s, **decisions) != re6.placed_expect(p, s)[1:]]
    print(what, "changes", changed)
    assert caught_by in changed
    good, bad = re6.placed_expect(re6.PLACED[caught_by], scale)[1:], _rule(re6.PLACED[caught_by], scale, **decisions)
    # far beyond the GPU file's bars: delta to 4 ulp, outliers exact
    assert abs(bad[0] - good[0]) > 1e-6 * good[0] or bad[1] != good[1]


def test_the_strict_mutant_needs_a_gap():
    """The grouped-data median is continuous in the counts: where `half` is met at a bin's end and the next bin holds rows
    too, 'reaches' and 'exceeds' give the same m, so only the placements with empty bins behind tell them apart."""
    strict = dict(reached=lambda cum, half: cum > half)
    for name, p in re6.PLACED.items():
        if name.startswith("half at the end") and not name.endswith("one moved"):
            same = _rule(p, 1.0, **strict) == re6.placed_expect(p, 1.0)[1:]
            assert same != name.endswith("then a gap"), name


# ---- B. objective 5's edge fixtures under the robust checker -------------------------------------------------------------
def _footed(what, pyr, K, cfg, init=None, lost=False):
    """The footing of one fixture: under the default scale factor the distances that exact counts need, the flat bar and
    the angle keep-outs; under UNIT_SCALE no weight but 1 on any iteration, and objective 5's checker's result."""
    ref = rr.optimize(pyr, K, cfg, init_pose=init)
    assert not re6.footing(ref), (what, re6.footing(ref))
    with re6.weights_heard() as heard:
        unit = rr.optimize(pyr, K, cfg, scale_factor=re6.UNIT_SCALE, init_pose=init)
    plain = ir.optimize(pyr, K, cfg, init)
    assert heard and not any(heard), (what, heard)
    assert len(heard) == sum(it for it, m in zip(unit["iterations"], cfg["max_iter"]) if m > 0)
    assert unit["outliers"] == [0] * cfg["num_levels"]
    assert (unit["iterations"], unit["valid_pixels"], unit["flags"]) == (plain["iterations"], plain["valid_pixels"],
                                                                         plain["flags"]), what
    if lost:
        for res in (ref, unit, plain):
            assert not np.any(np.isfinite(res["state"])), what
        return ref
    # the same rows and the same solve; g and H are summed by other BLAS calls (J^T r against (1 J)^T r): cond(H) <= 1e5
    # times a few units of 2^-53 stays far below 1e-10
    assert np.abs(unit["state"] - plain["state"]).max() <= 1e-10, what
    for res in (ref, plain):
        assert ie.flat(res), (what, res["cond"])
        assert ie.clear_of_the_cuts(res["state"]), (what, res["state"])
    assert plain["margin"] > ie.MARGIN_FLOOR, what
    return ref


@pytest.mark.parametrize("depth_range", ie.RANGES, ids=["default_range", "range_0.5_2"])
@pytest.mark.parametrize("w,h", list(ie.EXACT_SIZES), ids=["24x20", "75x53"])
def test_exact_positions_keep_their_footing(w, h, depth_range):
    bands = set()
    for shift in ie.EXACT_SIZES[(w, h)]:
        K, planes, state = ie.exact_problem(w, h, shift, depth_range)
        ref = _footed((w, h, shift, depth_range), [planes], K, ie.cfg([1], None, *depth_range), state)
        assert ref["valid_pixels"] == [ie.exact_rows(planes[1], shift)] and ref["flags"] == 0 and ref["outliers"][0] > 0
        bands |= ie.bands_seen(planes, K, state, depth_range)[0]
    assert bands == {"c-", "c+", "r-", "r+"}


@pytest.mark.parametrize("shift", ie.K_SHIFTS, ids=["ox+_oy-", "ox-_oy+"])
@pytest.mark.parametrize("w,h", ie.K_SIZES, ids=["75x53", "80x60"])
def test_intrinsics_fixtures_keep_their_footing_and_tell_fx_from_fy(w, h, shift):
    p, K = ie.intrinsics_problem(w, h, shift)
    pyr = ie.oracle_pyramid(p, 2)
    config = ie.cfg(ie.K_MAX_ITER)
    ref = _footed((w, h, shift), pyr, K, config, ie.K_INIT)
    assert ref["flags"] == 0 and ref["iterations"] == ie.K_MAX_ITER and min(ref["valid_pixels"]) > 500
    bar = rr.pose_bar(ref["cond"], ref["state"])
    for kind in ie.ROW_MUTANTS:
        with ie.row_focal_mutant(kind):
            alt = rr.optimize(pyr, K, config, init_pose=ie.K_INIT)
        dist = np.abs(alt["state"] - ref["state"]).max()
        print(f"{w}x{h} {shift} {kind}: {dist:.2e} = {dist / bar:.3g} bars")
        assert dist > 1e3 * bar, (kind, dist)
    assert np.array_equal(rr.optimize(pyr, K, config, init_pose=ie.K_INIT)["state"], ref["state"])


@pytest.mark.parametrize("layout", ie.ROWS_LAYOUTS)
def test_few_row_systems_keep_their_footing(layout):
    seed = ie.ROWS_SEED[layout]
    for count in (6, 7):
        for mi in ([1], [ie.ROWS_ITER]):
            K, planes = ie.rows_problem(seed, layout, count)
            ref = _footed((layout, count, mi), [planes], K, ie.cfg(mi))
            assert ref["valid_pixels"] == [count] and ref["flags"] == 0 and ref["iterations"] == mi
    for count, flags in ((5, BOTH), (6, ir.PAIR_NONFINITE)):
        K, planes = ie.rows_problem(seed, layout, count, constant_source=True)
        ref = _footed((layout, "constant", count), [planes], K, ie.cfg([ie.ROWS_ITER]), lost=True)
        assert ref["valid_pixels"] == [count] and ref["iterations"] == [1] and ref["flags"] == flags
        assert ref["delta"][0] > 0                                          # the rows are there: the histogram has them


def test_the_healthy_pairs_among_the_small_systems_keep_their_footing():
    for i, p in enumerate(ie.work_queue_pairs()[:ie.WQ_D]):
        ref = _footed(("healthy", i), ie.twin_pyramid(p, 1), p["K"], ie.cfg([ie.ROWS_ITER]))
        assert ref["flags"] == 0 and ref["outliers"][0] > 0


def test_edge_states_keep_their_footing():
    p = ie.angle_pair()
    pyr = ie.twin_pyramid(p, 2)
    finite = 0
    for s in edge_states.initial_states():
        lost = not np.all(np.isfinite(ir.optimize(pyr, p["K"], ie.cfg(ie.ANGLE_MAX_ITER), s)["state"]))
        ref = _footed(("state", s), pyr, p["K"], ie.cfg(ie.ANGLE_MAX_ITER), s, lost=lost)
        finite += not lost
        if lost:
            assert ref["valid_pixels"] == [0, 0] and ref["flags"] == BOTH and ref["delta"] == [0.0, 0.0]
    assert finite == ie.ANGLE_FINITE
    states, bad = ie.nonfinite_batch()
    for k, s in enumerate(states):
        ref = _footed(("position", k), pyr, p["K"], ie.cfg(ie.ANGLE_MAX_ITER), s, lost=k in bad)
        assert (ref["flags"] != 0) == (k in bad)


def test_large_motions_keep_their_footing():
    for p, init in ie.motion_pairs():
        ref = _footed(p["motion"][3], ie.twin_pyramid(p, 1), p["K"], ie.cfg(ie.MOTION_MAX_ITER, ie.MOTION_MIN_GRAD), init)
        assert ref["flags"] == 0 and 1 < ref["iterations"][0] < ie.MOTION_MAX_ITER[0]      # ended by its threshold
        assert abs(ref["state"][3] - p["motion"][3]) < 0.05


@pytest.mark.parametrize("lam", ie.STEP_LAMS, ids=["lam_0.7_0.5", "lam_1.0_0.7"])
def test_step_length_fixtures_keep_their_footing_and_depend_on_lambda(lam):
    small, wide = ie.step_pairs()
    for p, is_wide in [(q, False) for q in small] + [(wide, True)]:
        pyr = ie.oracle_pyramid(p, 2)
        for name, mi, mg in ie.step_configs(is_wide):
            ref = _footed((is_wide, name, lam), pyr, p["K"], ie.cfg(mi, mg, lam=lam))
            assert ref["flags"] == 0
            if name == "threshold":
                assert all(1 < it < m for it, m in zip(ref["iterations"], mi)), ref["iterations"]
            bar = rr.pose_bar(ref["cond"], ref["state"])
            for other in ([1.0, 1.0], lam[::-1]):
                alt = rr.optimize(pyr, p["K"], ie.cfg(mi, mg, lam=other))
                assert np.abs(alt["state"] - ref["state"]).max() > 1e3 * bar, (is_wide, name, lam, other)


# ---- C. levels -------------------------------------------------------------------------------------------------------------
def test_skipped_level_reports_nothing():
    p = ie.skip_pair()
    pyr = ie.twin_pyramid(p, 3)
    skip = _footed("skip", pyr, p["K"], ie.cfg(ie.SKIP_MAX_ITER))
    full = _footed("full", pyr, p["K"], ie.cfg(ie.FULL_MAX_ITER))
    assert skip["iterations"] == [5, 1, 5] and skip["valid_pixels"][1] == 0
    assert skip["delta"][1] == 0.0 and skip["outliers"][1] == 0
    assert full["iterations"] == [5, 5, 5] and full["delta"][1] > 0.0 and full["outliers"][1] > 0      # what would be left over
    assert min(skip["outliers"][0], skip["outliers"][2]) > 0
    assert np.abs(skip["state"] - full["state"]).max() > 1e3 * rr.pose_bar(full["cond"], full["state"])


def test_long_level_keeps_its_footing_and_stays_orthonormal():
    p = ie.long_pair()
    pyr = ie.twin_pyramid(p, 1)
    _footed("long", pyr, p["K"], ie.cfg([ie.LONG_ITER]))
    ref, R = re6.final_rotation(pyr, p["K"], ie.cfg([ie.LONG_ITER]))
    assert ref["iterations"] == [ie.LONG_ITER] and ref["flags"] == 0
    assert np.abs(R.T @ R - np.eye(3)).max() < ie.ORTHONORMAL_BELOW
    assert np.array_equal(ir.state_from_pose(R, ref["state"][:3]), ref["state"])


@pytest.mark.parametrize("w,h", list(re6.CHUNK_SIZES), ids=[f"{w}x{h}" for w, h in re6.CHUNK_SIZES])
def test_chunk_count_pairs_are_the_first_seeds_with_a_footing(w, h):
    assert re6.chunks_per_wave(w, h) == re6.CHUNK_SIZES[(w, h)]
    for seed in re6.CHUNK_SEARCH:
        p = cases.small_pair(seed, w, h)
        ref = rr.optimize(ie.oracle_pyramid(p, 1), p["K"], ie.cfg(re6.CHUNK_MAX_ITER))
        if (not re6.footing(ref) and ref["flags"] == 0 and ie.flat(ref) and np.abs(ref["state"][3:]).max() < 0.5
                and min(ref["outliers"]) > 0):
            break
    assert seed == re6.CHUNK_SEED[(w, h)]
    p = re6.chunk_pair(w, h)
    _footed(("chunks", w, h), ie.oracle_pyramid(p, 1), p["K"], ie.cfg(re6.CHUNK_MAX_ITER))


def test_the_chunk_counts_are_the_ones_the_parity_sizes_lack():
    assert [v[0] for v in re6.CHUNK_SIZES.values()] == [3, 3, 4, 1]
    assert re6.CHUNK_SIZES[(24, 24)][1:] == [2, 2, 2] and re6.CHUNK_SIZES[(26, 32)][1:] == [3, 3, 3]       # both exits in one pass
    assert re6.CHUNK_SIZES[(12, 10)][2:] == [0, 0]                          # two waves idle
