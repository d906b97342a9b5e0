"""CPU pre-checks of the inputs of tests/test_gpu_inverse_edges.py (tests/inverse_edges.py), on the CPU pyramids of
oracle/numpy_twin.py and oracle/oracle.py: every fixture the GPU file holds to the flat bar has cond(J^T J) <= 1e5 in the
checker (inverse_ref.pose_bar is then 1e-9 x max(1, |x|)), stays MARGIN_FLOOR clear of its gradient thresholds and ends
with yaw and roll 1e-3 clear of +-pi and pitch 0.05 clear of +-pi/2; row counts, flags and iteration patterns are the
expected ones; and the checker with a wrong step length or a wrong focal length in its row -- what the fixtures of parts E
and F exist to catch -- ends more than a thousand bars away.  No GPU."""
import numpy as np
import pytest

import edge_states
import inverse_edges as ie
import inverse_ref as ir

BOTH = ir.PAIR_RANK_DEFICIENT | ir.PAIR_NONFINITE


def _holds(ref, what):
    assert np.all(np.isfinite(ref["state"])), what
    assert ie.flat(ref), (what, ref["cond"])
    assert ref["margin"] > ie.MARGIN_FLOOR, (what, ref["margin"])
    assert ie.clear_of_the_cuts(ref["state"]), (what, ref["state"])


def test_the_keep_out_margins_are_the_stated_ones():
    assert (ie.MARGIN_FLOOR, ie.YAW_ROLL_KEEP_OUT, ie.PITCH_KEEP_OUT) == (1e-6, 1e-3, 0.05)
    base = np.array([0.0, 0.0, 0.0, 0.1, 0.2, 0.3])
    assert ie.clear_of_the_cuts(base)
    for k, v in ((3, np.pi - 5e-4), (3, -np.pi + 5e-4), (5, np.pi - 5e-4), (4, 0.5 * np.pi - 0.04), (4, -0.5 * np.pi + 0.04)):
        s = base.copy()
        s[k] = v
        assert not ie.clear_of_the_cuts(s), (k, v)


# ---- A. the work queue ---------------------------------------------------------------------------------------------
def test_work_queue_pairs_hold_the_flat_bar_from_every_start():
    pairs = ie.work_queue_pairs()
    cfg = ie.cfg(ie.WQ_MAX_ITER, ie.WQ_MIN_GRAD)
    which = ie.work_queue_list(1541)
    assert 0.07 < np.mean(which == ie.WQ_D) < 0.13 and set(which.tolist()) == {0, 1, 2, 3}
    states, pick = ie.work_queue_inits(520)
    assert np.all(states != 0.0) and set(pick.tolist()) == set(range(ie.WQ_INITS)) and len(states) == 6
    alone, every = [], set()
    for i, p in enumerate(pairs):
        pyr = ie.twin_pyramid(p, ie.WQ_LEVELS)
        assert [lv[0].size for lv in pyr] == [480, 120]
        for init in [None] + list(states):
            ref = ir.optimize(pyr, p["K"], cfg, init_pose=init)
            if i == ie.WQ_D:
                assert ref["valid_pixels"] == [0, 0] and ref["flags"] == BOTH and ref["iterations"] == [1, 1]
                assert np.all(np.isnan(ref["state"]))
                continue
            _holds(ref, (i, init))
            assert ref["flags"] == 0 and all(1 < it < 8 for it in ref["iterations"]), ref["iterations"]   # by the thresholds
            every.add(tuple(ref["iterations"]))
            if init is None:
                alone.append(tuple(ref["iterations"]))
    print(alone, sorted(every))
    assert len(set(alone)) >= 2 and len(every) >= 3           # the pairs differ in the work they take


# ---- B. exact positions ------------------------------------------------------------------------------------------------
# (w, h, range) -> rows at +-0.25 and at +-0.5 / +-0.75 (affine_edges' planes: the counts of test_affine_edges_cpu.py)
EXACT_ROWS = {(24, 20, (0.3, 5.0)): (437, 396), (24, 20, (0.5, 2.0)): (396, 357),
              (75, 53, (0.3, 5.0)): (3848, 3723), (75, 53, (0.5, 2.0)): (3723, 3600)}


@pytest.mark.parametrize("depth_range", ie.RANGES, ids=["default_range", "range_0.5_2"])
@pytest.mark.parametrize("w,h", list(ie.EXACT_SIZES), ids=["24x20", "75x53"])
def test_exact_positions_rows_bands_and_conditioning(w, h, depth_range):
    conds = []
    for shift in ie.EXACT_SIZES[(w, h)]:
        K, planes, state = ie.exact_problem(w, h, shift, depth_range)
        expected = ie.exact_rows(planes[1], shift)
        assert expected == EXACT_ROWS[(w, h, depth_range)][0 if abs(shift) == 0.25 else 1], (shift, expected)
        seen, rows = ie.bands_seen(planes, K, state, depth_range)
        assert rows == expected
        assert seen == ie.exact_bands(shift), (shift, seen)     # clamped taps exactly at +-0.25
        ref = ir.optimize([planes], K, ie.cfg([1], None, *depth_range), init_pose=state)
        assert ref["valid_pixels"] == [expected] and ref["iterations"] == [1] and ref["flags"] == 0
        _holds(ref, (w, h, shift, depth_range))
        conds.append(ref["cond"])
    print(f"{w}x{h} {depth_range}: cond {min(conds):.2e} ... {max(conds):.2e}")
    assert max(conds) < 1e5


# ---- C. Exp's three regimes ------------------------------------------------------------------------------------------
def test_exp_regimes_are_all_met_and_end_clear_of_the_cuts():
    """27 cases: per target the side of the Taylor switch and the branches lane 0 (th) and lane 1 (th / 2) take; every
    result finite, flags 0, flat bar; the output is state_from_pose(Exp(xi)) itself."""
    expected = {5e-5: (True, False, False), 9.9e-5: (True, False, False), 1.01e-4: (False, False, False),
                0.3: (False, False, False), 0.783: (False, False, False), 0.80: (False, True, False),
                1.2: (False, True, False), 2.0: (False, True, True), 3.0: (False, True, True)}
    assert tuple(expected) == ie.EXP_TARGETS
    rows, conds, largest = [], [], 0.0
    for seed in ie.EXP_SEEDS:
        p = ie.exp_pair(seed)
        pyr = ie.twin_pyramid(p, 1)
        for target in ie.EXP_TARGETS:
            lam, xi = ie.exp_lambda(pyr[0], p["K"], target)
            assert ie.exp_regime(xi) == expected[target], (seed, target, ie.exp_regime(xi))
            assert abs(np.linalg.norm(xi[3:]) - target) <= 1e-12 * target
            ref = ir.optimize(pyr, p["K"], ie.cfg([1], lam=[lam]))
            _holds(ref, (seed, target))
            assert ref["flags"] == 0 and ref["iterations"] == [1]
            ER, Et = ir.se3_exp(xi)
            assert np.abs(ref["state"] - ir.state_from_pose(ER, Et)).max() <= 1e-12 * max(1.0, np.abs(ref["state"]).max())
            rows.append(ref["valid_pixels"][0])
            conds.append(ref["cond"])
            largest = max(largest, float(np.abs(ref["state"][3:]).max()))
    print(f"rows {min(rows)} ... {max(rows)}, cond {min(conds):.2e} ... {max(conds):.2e}, largest output angle {largest:.3f}")
    assert largest > 2.0                                        # atan2 far outside its first octant


# ---- D. large angles ---------------------------------------------------------------------------------------------------
def test_edge_states_split_into_finite_and_lost():
    p = ie.angle_pair()
    pyr = ie.twin_pyramid(p, 2)
    finite, lost, conds = 0, [], []
    for s in edge_states.initial_states():
        ref = ir.optimize(pyr, p["K"], ie.cfg(ie.ANGLE_MAX_ITER), init_pose=s)
        if np.all(np.isfinite(ref["state"])):
            _holds(ref, s)
            finite += 1
            conds.append(ref["cond"])
        else:
            assert ref["valid_pixels"] == [0, 0] and ref["flags"] == BOTH and np.all(np.isnan(ref["state"]))
            lost.append(s)
    print(f"cond {min(conds):.2e} ... {max(conds):.2e}")
    assert (finite, len(lost)) == (ie.ANGLE_FINITE, ie.ANGLE_LOST) and finite + len(lost) == 32
    assert sorted(float(s[3:][np.argmax(np.abs(s[3:]))]) for s in lost) == [-1.2, -1.2, 1.2, 1.2]
    assert all(int(np.argmax(np.abs(s[3:]))) in (1, 2) for s in lost)      # pitch or roll


def test_large_motions_and_nonfinite_starts():
    for p, init in ie.motion_pairs():
        ref = ir.optimize(ie.twin_pyramid(p, 1), p["K"], ie.cfg(ie.MOTION_MAX_ITER, ie.MOTION_MIN_GRAD), init_pose=init)
        _holds(ref, p["motion"][3])
        print(f"yaw {p['motion'][3]}: iterations {ref['iterations']}, cond {ref['cond']:.2e}")
        assert ref["flags"] == 0 and 1 < ref["iterations"][0] < ie.MOTION_MAX_ITER[0]
        assert abs(ref["state"][3] - p["motion"][3]) < 0.05
    p = ie.angle_pair()
    pyr = ie.twin_pyramid(p, 2)
    states, bad = ie.nonfinite_batch()
    assert len(states) == 10 and bad == [3, 7] and np.isnan(states[3][3]) and np.isinf(states[7][3])
    for k, s in enumerate(states):
        ref = ir.optimize(pyr, p["K"], ie.cfg(ie.ANGLE_MAX_ITER), init_pose=s)
        if k in bad:
            assert ref["iterations"] == [1, 1] and ref["valid_pixels"] == [0, 0]
            assert ref["flags"] & ir.PAIR_NONFINITE and np.all(np.isnan(ref["state"]))
        else:
            _holds(ref, k)
            assert ref["flags"] == 0


# ---- E. step length ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", ie.STEP_LAMS, ids=["lam_0.7_0.5", "lam_1.0_0.7"])
def test_step_length_fixtures_depend_on_lambda(lam):
    """Flat bar and threshold margin as everywhere; and the checker's own result under lambda = 1 on every level, or under
    the two levels' lambdas exchanged, is further away than a thousand bars: a kernel that ignored lambda or took another
    level's cannot pass."""
    small, wide = ie.step_pairs()
    nearest = np.inf
    for p, is_wide in [(q, False) for q in small] + [(wide, True)]:
        pyr = ie.oracle_pyramid(p, 2)
        if not is_wide:
            twin = ie.twin_pyramid(p, 2)
            assert all(np.array_equal(a, b) for lv, lt in zip(pyr, twin) for a, b in zip(lv, lt))
        for name, mi, mg in ie.step_configs(is_wide):
            ref = ir.optimize(pyr, p["K"], ie.cfg(mi, mg, lam=lam))
            _holds(ref, (is_wide, name, lam))
            assert ref["flags"] == 0
            if name == "threshold":
                assert all(1 < it < m for it, m in zip(ref["iterations"], mi)), ref["iterations"]   # thresholds end both levels
            else:
                assert ref["iterations"] == mi
            bar = ir.pose_bar(ref["cond"], ref["state"])
            for other in ([1.0, 1.0], lam[::-1]):
                alt = ir.optimize(pyr, p["K"], ie.cfg(mi, mg, lam=other))
                ratio = np.abs(alt["state"] - ref["state"]).max() / bar
                nearest = min(nearest, ratio)
                assert ratio > 1e3, (is_wide, name, lam, other, ratio)
    print(f"lambda {lam}: the nearest mutant is {nearest:.3g} bars away")


# ---- F. intrinsics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ie.K_SHIFTS, ids=["ox+_oy-", "ox-_oy+"])
@pytest.mark.parametrize("w,h", ie.K_SIZES, ids=["75x53", "80x60"])
def test_intrinsics_fixtures_tell_fx_from_fy_in_the_row(w, h, shift):
    """fy = 1.1 fx: a row that takes fx for both image-gradient columns, fy for both, or the two exchanged -- the warp left
    right -- ends more than a thousand bars away."""
    p, K = ie.intrinsics_problem(w, h, shift)
    assert K[1, 1] == 1.1 * K[0, 0] and (K[0, 2] * 2) % 1 != 0 and (K[1, 2] * 2) % 1 != 0
    pyr = ie.oracle_pyramid(p, 2)
    config = ie.cfg(ie.K_MAX_ITER)
    ref = ir.optimize(pyr, K, config, init_pose=ie.K_INIT)
    _holds(ref, (w, h, shift))
    assert ref["flags"] == 0 and ref["iterations"] == ie.K_MAX_ITER and min(ref["valid_pixels"]) > 500
    bar = ir.pose_bar(ref["cond"], ref["state"])
    for kind in ie.ROW_MUTANTS:
        with ie.row_focal_mutant(kind):
            alt = ir.optimize(pyr, K, config, init_pose=ie.K_INIT)
        dist = np.abs(alt["state"] - ref["state"]).max()
        print(f"{w}x{h} {shift} {kind}: {dist:.2e} = {dist / bar:.3g} bars, cond {ref['cond']:.2e}")
        assert dist > 1e3 * bar, (kind, dist)
    again = ir.optimize(pyr, K, config, init_pose=ie.K_INIT)      # the wrapper left the checker as it was
    assert np.array_equal(again["state"], ref["state"])


# ---- G. five, six and seven rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ie.ROWS_LAYOUTS)
def test_six_and_seven_row_problems_are_the_best_of_their_seed_range(layout):
    """The committed seed is the one the search over ROWS_SEARCH finds; its 6- and 7-row systems keep their rows over
    ROWS_ITER iterations under the flat bar; the rows sit where the layout says; the constant-source systems of 5 and 6
    rows have an exactly zero H and the flags that follow from the row count alone."""
    conds = [ie.rows_worst_cond(s, layout) for s in ie.ROWS_SEARCH]
    seed = int(np.argmin(conds))
    usable = int(np.sum(np.array(conds) <= 1e5))
    print(layout, seed, conds[seed], "usable", usable)
    assert seed == ie.ROWS_SEED[layout] and conds[seed] <= 1e3, (seed, conds[seed])
    assert usable == dict(one_chunk=222, four_waves=245)[layout]
    for count in (6, 7):
        K, planes = ie.rows_problem(seed, layout, count)
        chunks = [int(k) // 64 for k in np.flatnonzero(np.isfinite(planes[1]).reshape(-1))]
        assert len(chunks) == count
        if layout == "one_chunk":
            assert set(chunks) == {2}
        else:
            assert {c % 4 for c in chunks} == {0, 1, 2, 3}      # rows of all four waves
        for mi in ([1], [ie.ROWS_ITER]):
            ref = ir.optimize([planes], K, ie.cfg(mi))
            _holds(ref, (layout, count, mi))
            assert ref["valid_pixels"] == [count] and ref["flags"] == 0 and ref["iterations"] == mi
    for count, flags in ((5, BOTH), (6, ir.PAIR_NONFINITE)):
        K, planes = ie.rows_problem(seed, layout, count, constant_source=True)
        assert not planes[2].any() and not planes[3].any()
        g, Hm, n = ir.system(planes, 0, K, np.eye(3), np.zeros(3))
        assert n == count and not Hm.any() and not g.any()
        ref = ir.optimize([planes], K, ie.cfg([ie.ROWS_ITER]))
        assert ref["valid_pixels"] == [count] and ref["iterations"] == [1] and ref["flags"] == flags
        assert np.all(np.isnan(ref["state"]))


def test_the_mixed_row_systems_are_the_four_of_the_issue():
    got = []
    for name, layout, count, const in ie.ROWS_MIXED:
        K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
        ref = ir.optimize([planes], K, ie.cfg([ie.ROWS_ITER]))
        got.append((count, const, ref["flags"]))
    assert got == [(6, False, 0), (5, True, BOTH), (7, False, 0), (6, True, ir.PAIR_NONFINITE)]


# ---- H. a skipped level and a long level ---------------------------------------------------------------------------------
def test_skipped_level_does_nothing():
    p = ie.skip_pair()
    pyr = ie.twin_pyramid(p, 3)
    skip = ir.optimize(pyr, p["K"], ie.cfg(ie.SKIP_MAX_ITER))
    full = ir.optimize(pyr, p["K"], ie.cfg(ie.FULL_MAX_ITER))
    for ref in (skip, full):
        _holds(ref, ref["iterations"])
        assert ref["flags"] == 0
    print(f"cond {skip['cond']:.2e}, {full['cond']:.2e}")
    assert skip["iterations"] == [5, 1, 5] and skip["valid_pixels"][1] == 0 and full["iterations"] == [5, 5, 5]
    bar = ir.pose_bar(full["cond"], full["state"])
    assert np.abs(skip["state"] - full["state"]).max() > 1e3 * bar      # the middle level's five iterations are missing


def test_long_level_stays_orthonormal():
    """50 compositions without re-orthonormalisation: |R^T R - I| of the checker's final rotation is below 1e-13, four
    orders under the 1e-9 bar, so drift is not what the bar absorbs."""
    p = ie.long_pair()
    pyr = ie.twin_pyramid(p, 1)
    ref, R = ie.final_rotation(pyr, p["K"], ie.cfg([ie.LONG_ITER]))
    _holds(ref, "long level")
    assert ref["iterations"] == [ie.LONG_ITER] and ref["flags"] == 0 and ie.LONG_ITER == 50
    drift = np.abs(R.T @ R - np.eye(3)).max()
    print(f"|R^T R - I| = {drift:.2e}, cond {ref['cond']:.2e}")
    assert drift < ie.ORTHONORMAL_BELOW == 1e-13
    assert np.array_equal(ir.state_from_pose(R, ref["state"][:3]), ref["state"])
