"""phovo_engine_evaluate_robust_pairs and phovo_odometry_get_robust_system on the device: the weighted
twist-basis system of the robust inverse-compositional objective against the numpy checker (tests/robust_system_ref.py) fed
the planes exactly as the device holds them (get_level_planes), never the code under test.  The bars are the project's own:
H within 1e-10 of its scale and g within 1e-9 sqrt(H_ii cost) (sampled_system_ref.check_against), each of the three costs
within 1e-12 relative, delta and median within 4 ulp, rows, outliers and flags exact, H exactly symmetric.  Counts can be
exact only away from the bin edges and from delta: every comparison first asserts the checker's margins on the device's own
planes (1e-7 bins, 1e-10 in |r| - delta).  The fixtures are tests/robust_system_cases.py's; tests/test_robust_system_cpu.py
holds them to what this file relies on without a device."""
import ctypes as C

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

import inverse_edges as ie
import inverse_ref as ir
import inverse_robust_cases as rc
import inverse_robust_edges as re_
import inverse_robust_ref as rr
import inverse_system_ref as isr
import robust_system_cases as cs
import robust_system_ref as rsr

pytestmark = pytest.mark.gpu

ROBUST = native.OBJECTIVE_INVERSE_ROBUST
INVERSE = native.OBJECTIVE_INVERSE_COMPOSITIONAL


def _engine(K, w, h, nl=1, frames=2, depth_range=None, max_iter=None, lam=None, scale=None):
    eng = odometry.AlignmentEngine()
    eng.set_config(native.make_config(num_levels=nl, max_iter=max_iter if max_iter else [1] * nl, min_grad=[0.0] * nl, lam=lam))
    eng.set_objective(ROBUST)
    if scale is not None:
        eng.set_robust_options(native.make_robust_options(scale))
    eng.set_intrinsic_matrix(K)
    if depth_range is not None:
        eng.set_depth_range(*depth_range)
    eng.reserve_frames(frames, w, h)
    return eng


def _pair_engine(p, nl=1, **kw):
    h, w = p["gray0"].shape
    eng = _engine(p["K"], w, h, nl, **kw)
    eng.upload_frame(0, p["gray0"], p["depth0"])
    eng.upload_frame(1, p["gray1"], p["depth1"])
    return eng


def _set_planes(eng, planes, src=0, tgt=1):
    """One level plane by plane: the source's four planes, the target's intensity (and zero gradient planes, which no row
    reads: writing them gives the frame its target role on the level)."""
    i0, d0, gx0, gy0, i1 = planes
    eng.set_level_planes(src, 0, intensity=i0, depth=d0, grad_x=gx0, grad_y=gy0)
    eng.set_level_planes(tgt, 0, intensity=i1, grad_x=np.zeros_like(i1), grad_y=np.zeros_like(i1))


def _planes(eng, level, src=0, tgt=1):
    i0, d0, gx0, gy0 = eng.get_level_planes(src, level)
    i1, _, _, _ = eng.get_level_planes(tgt, level)
    return i0, d0, gx0, gy0, i1


def _bytes(structs):
    return [bytes(memoryview(r)) for r in structs]


def _evaluate(eng, states, level=0, src=0, tgt=1, deltas=None, **kw):
    states = np.atleast_2d(np.asarray(states, dtype=np.float64))
    n = len(states)
    return eng.evaluate_robust_pairs([src] * n, [tgt] * n, states, level, deltas=deltas, **kw)


def _hold(part, rec, planes, level, K, states, scale=rr.DEFAULT_SCALE, depth_range=(0.3, 5.0), deltas=None):
    """Every record of `rec` against the checker; prints the part's worst distances over bar."""
    worst = (0.0, 0.0)
    for k, st in enumerate(np.atleast_2d(states)):
        ref = rsr.system(planes, level, K, st, scale, *depth_range, delta=None if deltas is None else deltas[k])
        try:
            dh, dg = rsr.check_record(rec, k, ref, given=deltas is not None)
        except AssertionError as err:
            raise AssertionError(f"{part}, state {k}: {err}") from err
        worst = (max(worst[0], dh), max(worst[1], dg))
    print(f"{part}: worst dH / bar {worst[0]:.3g}, dg / bar {worst[1]:.3g}; rows {list(rec['rows'])} outliers "
          f"{list(rec['outliers'])} delta {list(rec['delta'])}")
    return worst


# ---- tile geometries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", cs.GEOMETRIES, ids=["%dx%d" % s for s in cs.GEOMETRIES])
def test_tile_geometries(w, h):
    p = cs.geometry_pair(w, h)
    states = cs.three_states(p)
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        rec = _evaluate(eng, states)
    _hold(f"geometry {w}x{h}", rec, planes, 0, p["K"], states)
    if cs.well_posed_size(w, h):
        assert np.all(rec["rows"] >= 6) and not rec["flags"].any() and np.all(rec["outliers"] > 0)


def test_one_vga_level():
    p = cs.vga_pair()
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        rec = _evaluate(eng, p["motion"])
    _hold("640x480", rec, planes, 0, p["K"], p["motion"])
    assert rec["rows"][0] > 250000 and rec["flags"][0] == 0


def test_the_occluded_pair():
    p = cs.occluded_pair()
    states = cs.three_states(p)
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        rec = _evaluate(eng, states)
    _hold("160x120 occluded", rec, planes, 0, p["K"], states)
    assert np.all(rec["outliers"] > 0.05 * rec["rows"])
    assert np.all(rec["cost"] < rec["huber_cost"]) and np.all(rec["huber_cost"] < rec["squared_cost"])


# ---- placed medians ----------------------------------------------------------------------------------------------------
def _placed_check(what, rec, k, expect):
    rows, delta, outliers = expect
    assert rec["rows"][k] == rows, (what, rec["rows"][k], rows)
    assert rsr.ulps(rec["delta"][k], delta) <= rsr.ULPS, (what, rec["delta"][k], delta)
    assert rec["outliers"][k] == outliers, (what, rec["outliers"][k], outliers)
    assert np.array_equal(rec["information"][k], rec["information"][k].T)


def test_placed_medians_alone_and_in_one_call():
    """All 59 placements of inverse_robust_edges.PLACED at the zero state against placed_expect, under the default scale
    factor, 0.5 and 1.0 (the ties are inliers): each alone, and all of them as one call of 59 pairs -- the same bytes."""
    names = re_.PLACED_NAMES
    assert len(names) == 59
    zero = np.zeros((len(names), 6))
    with _engine(rc.EDGE_K, rc.EDGE_W, rc.EDGE_H, frames=2 * len(names)) as eng:
        for i, name in enumerate(names):
            _set_planes(eng, re_.placed_planes(name), 2 * i, 2 * i + 1)
        src, tgt = [2 * i for i in range(len(names))], [2 * i + 1 for i in range(len(names))]
        for scale in re_.PLACED_SCALES:
            eng.set_robust_options(native.make_robust_options(scale))
            rec = eng.evaluate_robust_pairs(src, tgt, zero, 0, want_structs=True)
            together = _bytes(rec["structs"])
            for i, name in enumerate(names):
                _placed_check((name, scale), rec, i, re_.placed_expect(re_.PLACED[name], scale))
                one = eng.evaluate_robust_pairs([src[i]], [tgt[i]], zero[:1], 0, want_structs=True)
                assert _bytes(one["structs"])[0] == together[i], (name, scale)
            if scale == re_.TIE_SCALE:
                for name in re_.PLACED_TIES:                     # |r| == delta exactly: inliers
                    assert rec["outliers"][names.index(name)] == (140 if name == "tie" else 0), name


def test_placed_medians_across_three_tiles():
    """The same (bin, count) lists with every count times 6 on 64x48 planes: three tiles, every bin's rows dealt to all of
    them, so the pair's histogram -- and the median -- exists only as the sum of the three tiles' flushes."""
    names = re_.PLACED_NAMES
    zero = np.zeros((len(names), 6))
    with _engine(cs.TILES_K, cs.TILES_W, cs.TILES_H, frames=2 * len(names)) as eng:
        for i, name in enumerate(names):
            _set_planes(eng, cs.tiles_planes(name)[0], 2 * i, 2 * i + 1)
        src, tgt = [2 * i for i in range(len(names))], [2 * i + 1 for i in range(len(names))]
        for scale in re_.PLACED_SCALES:
            eng.set_robust_options(native.make_robust_options(scale))
            rec = eng.evaluate_robust_pairs(src, tgt, zero, 0)
            for i, name in enumerate(names):
                _placed_check((name, scale, "three tiles"), rec, i, re_.placed_expect(cs.tiles_placement(name), scale))
                assert rec["median"][i] * scale == rec["delta"][i]


# ---- the aligner's first step is this system ---------------------------------------------------------------------------
@pytest.mark.parametrize("lam", cs.STEP_LAMS)
def test_the_aligners_first_step_is_this_system(lam):
    worst = 0.0
    for i, p in enumerate(cs.step_pairs()):
        for start in (np.zeros(6), cs.STEP_START):
            with _pair_engine(p, lam=[lam]) as eng:
                s, reps = eng.align_pairs([0], [1], init_states=start[None], want_reports=True)
                assert {l["kind"] for l in eng.last_launches()} == {"inverse_robust"}
                rob = eng.fetch_robust_reports(1)
                planes = _planes(eng, 0)
                rec = _evaluate(eng, start)
            ref = rsr.system(planes, 0, p["K"], start)
            assert rsr.margins_hold(ref), (i, ref["bin_margin"], ref["delta_margin"])
            assert rsr.ulps(rec["delta"][0], float(rob["delta"][0][0])) <= rsr.ULPS
            assert rec["outliers"][0] == rob["outliers"][0][0] and rec["rows"][0] == reps[0].valid_pixels[0]
            H, g = rec["information"][0], rec["gradient"][0]
            xi = -lam * np.linalg.solve(H, g)                                  # from the RECORD
            R, t = ir.eigen_rt(start)
            ER, Et = ir.se3_exp(xi)
            expect = ir.state_from_pose(R @ ER, R @ Et + t)
            bar = ir.pose_bar(float(np.linalg.cond(H)), expect)
            err = np.abs(s[0] - expect).max()
            worst = max(worst, err / bar)
            assert err <= bar, (i, start, err, bar)
            gn = float(np.linalg.norm(g))
            assert abs(reps[0].gradient_norm - gn) <= 1e-9 * gn
            assert list(reps[0].iterations[:1]) == [1]
    print(f"first step lambda {lam}: worst distance / bar {worst:.3g}")


# ---- given deltas ----------------------------------------------------------------------------------------------------
UNIT_FIELDS = ("information", "gradient", "rows", "flags", "cost", "huber_cost", "squared_cost")


def test_given_deltas():
    p = cs.geometry_pair(75, 53)
    states = cs.three_states(p)
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        own = _evaluate(eng, states, want_structs=True)
        _hold("75x53 computed", own, planes, 0, p["K"], states)
        # the record's own delta handed back: every field but the median, bit for bit
        again = _evaluate(eng, states, deltas=own["delta"], want_structs=True)
        assert np.all(again["median"] == 0.0) and np.all(own["median"] > 0.0)
        for a, b in zip(again["structs"], own["structs"]):
            b.median = 0.0
        assert _bytes(again["structs"]) == _bytes(own["structs"])
        # a small delta: most rows are outliers, against the checker
        small = cs.SMALL_DELTA_SHARE * own["median"]
        rec = _evaluate(eng, states, deltas=small)
        _hold("75x53 small delta", rec, planes, 0, p["K"], states, deltas=small)
        assert np.all(rec["outliers"] > 0.5 * rec["rows"]) and np.all(rec["cost"] < rec["squared_cost"])
        # different deltas in one call stay with their pairs
        mixed = np.array([small[0], own["delta"][1], cs.UNIT_DELTA])
        rec = _evaluate(eng, states, deltas=mixed)
        _hold("75x53 mixed deltas", rec, planes, 0, p["K"], states, deltas=mixed)
        assert list(rec["delta"]) == list(mixed) and rec["outliers"][2] == 0
        # bad entries are refused before any launch: the workspace and the last records are untouched, whatever the position
        s, t = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(1, 1, 1)
        st = np.ascontiguousarray(states)
        out = (native.RobustSystem * 3)()
        for bad in cs.BAD_DELTAS:
            for at in range(3):
                d = np.array([0.01, 0.01, 0.01])
                d[at] = bad
                got = eng._lib.phovo_engine_evaluate_robust_pairs(eng._h, 3, s, t, st.ctypes.data, d.ctypes.data, 0, out)
                assert got == native.E_INVALID_ARGUMENT, (bad, at)
                assert b"delta" in native.lib().phovo_last_error()
        assert all(o.rows == 0 and o.delta == 0.0 for o in out)


@pytest.mark.parametrize("make", [lambda: cs.geometry_pair(8, 8), lambda: cs.geometry_pair(41, 25), lambda: cs.geometry_pair(75, 53),
                                  cs.occluded_pair], ids=["8x8", "41x25", "75x53", "160x120_occluded"])
def test_a_delta_beyond_every_residual_gives_objective_5s_record_bit_for_bit(make):
    """deltas = 2^40: every weight is exactly 1, so w J = J and w r = r bit for bit, and the kernel adds the same rows in the
    same orders as k_eval_inverse: information, gradient, rows, flags and the three costs are
    phovo_engine_evaluate_inverse_pairs' under objective 5 on the same engine and frames, BIT FOR BIT on every fixture (DESIGN.md
    §23 records that none differed)."""
    p = make()
    states = cs.three_states(p)
    with _pair_engine(p) as eng:
        rec = _evaluate(eng, states, deltas=np.full(3, cs.UNIT_DELTA))
        eng.set_objective(INVERSE)
        n = len(states)
        inv = eng.evaluate_inverse_pairs([0] * n, [1] * n, states, 0)
        eng.set_objective(ROBUST)
        unit = _evaluate(eng, states)                             # and the same through the scale factor
        eng.set_robust_options(native.make_robust_options(cs.UNIT_SCALE))
        scaled = _evaluate(eng, states)
    assert np.all(rec["outliers"] == 0) and np.all(scaled["outliers"] == 0) and np.any(unit["outliers"] > 0)
    for r in (rec, scaled):
        for key in ("information", "gradient", "rows", "flags"):
            assert np.array_equal(r[key], inv[key]), key
        for key in rsr.COSTS:
            assert np.array_equal(r[key], inv["cost"]), key
    assert np.all(scaled["delta"] == cs.UNIT_SCALE * scaled["median"]) and np.all(scaled["median"] == unit["median"])


# ---- scale factor ----------------------------------------------------------------------------------------------------
def test_the_scale_factor():
    p = cs.geometry_pair(75, 53)
    states = cs.three_states(p)
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        recs = {}
        for scale in cs.SCALES + (cs.UNIT_SCALE,):
            eng.set_robust_options(native.make_robust_options(scale))
            recs[scale] = _evaluate(eng, states)
            _hold(f"75x53 scale {scale:.6g}", recs[scale], planes, 0, p["K"], states, scale)
    assert np.all(recs[0.5]["delta"] < recs[1.0]["delta"]) and np.all(recs[0.5]["outliers"] > recs[1.0]["outliers"])
    assert np.all(recs[0.5]["median"] == recs[1.0]["median"]) and np.all(recs[1.0]["delta"] == recs[1.0]["median"])
    assert np.all(recs[cs.UNIT_SCALE]["outliers"] == 0)
    assert np.array_equal(recs[cs.UNIT_SCALE]["cost"], recs[cs.UNIT_SCALE]["squared_cost"])


# ---- small systems, NaN ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,count,const", cs.ROWS_CASES)
def test_small_systems(layout, count, const):
    K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
    with _engine(K, ie.ROWS_W, ie.ROWS_H) as eng:
        _set_planes(eng, planes)
        held = _planes(eng, 0)
        rec = _evaluate(eng, np.zeros(6))
    _hold(f"{layout} {count} rows, constant source {const}", rec, held, 0, K, np.zeros(6))
    assert rec["rows"][0] == count
    assert rec["flags"][0] == (native.PAIR_RANK_DEFICIENT if count < 6 else 0)
    if const:                                                    # H exactly zero with finite sums
        assert not rec["information"][0].any() and not rec["gradient"][0].any() and np.isfinite(rec["cost"][0])


def test_all_nan_depth():
    p = cs.geometry_pair(75, 53)
    p["depth0"] = np.full_like(p["depth0"], np.nan)
    with _pair_engine(p) as eng:
        rec = _evaluate(eng, p["motion"], want_structs=True)
        given = _evaluate(eng, p["motion"], deltas=[0.01])
    assert rec["rows"][0] == 0 and rec["outliers"][0] == 0 and rec["flags"][0] == native.PAIR_RANK_DEFICIENT
    assert rec["median"][0] == 0.0 and rec["delta"][0] == 0.0 and all(rec[c][0] == 0.0 for c in rsr.COSTS)
    assert not rec["information"][0].any() and not rec["gradient"][0].any() and rec["structs"][0].reserved == 0
    assert given["rows"][0] == 0 and given["delta"][0] == 0.01 and given["flags"][0] == native.PAIR_RANK_DEFICIENT


def test_nan_in_the_source_gradient_and_in_the_target():
    p = cs.geometry_pair(75, 53)
    st = p["motion"] + cs.NAN_SHIFT
    with _pair_engine(p) as eng:
        planes = _planes(eng, 0)
        clean = _evaluate(eng, st)
        _hold("nan planes, clean", clean, planes, 0, p["K"], st)
        # NaN in 200 pixels of GX0 only: rows, delta, outliers and the costs are the clean record's, NONFINITE set
        eng.set_level_planes(0, 0, grad_x=cs.nan_gx_planes(planes)[2])
        rec = _evaluate(eng, st)
        _hold("nan in GX0", rec, _planes(eng, 0), 0, p["K"], st)
        assert rec["flags"][0] == native.PAIR_NONFINITE and clean["flags"][0] == 0
        for key in ("rows", "delta", "median", "outliers") + rsr.COSTS:
            assert rec[key][0] == clean[key][0], key
        assert np.isfinite(rec["information"][0][1, 1]) and not np.isfinite(rec["information"][0][0, 0])
        eng.set_level_planes(0, 0, grad_x=planes[2])
        # NaN in I1 pixels that rows sample: the NaN residuals are counted in the last bin, as the checker says
        hit = isr.sampled_target_pixels(planes, 0, p["K"], st)
        bad = cs.nan_i1_planes(planes, hit)
        eng.set_level_planes(1, 0, intensity=bad[4])
        held = _planes(eng, 0)
        rec = _evaluate(eng, st)
        ref = rsr.system(held, 0, p["K"], st)
        assert ref["last_bin"] > 0 and ref["rows"] == clean["rows"][0]
        _hold("nan in I1", rec, held, 0, p["K"], st)
        assert rec["flags"][0] == native.PAIR_NONFINITE and not np.isfinite(rec["squared_cost"][0])


# ---- bit identity --------------------------------------------------------------------------------------------------------
def test_bit_identical_alone_in_a_batch_and_under_every_setting():
    x, y = cs.geometry_pair(75, 53), ie.long_pair()
    y = {k: np.ascontiguousarray(v[:53, :75]) for k, v in y.items() if k != "K" and k != "motion"}
    st = np.asarray(x["motion"])
    with _pair_engine(x, frames=4, max_iter=[3]) as eng:
        eng.upload_frame(2, y["gray0"], y["depth0"])
        eng.upload_frame(3, y["gray1"], y["depth1"])

        def alone(deltas=None):
            return _bytes(eng.evaluate_robust_pairs([0], [1], st[None], 0, deltas=deltas, want_structs=True)["structs"])[0]
        first = alone()
        assert alone() == first                                   # twice in a row: the histograms are cleared between calls
        rs = np.random.RandomState(1)
        src, tgt, states = [2] * 64, [3] * 64, rs.uniform(-0.02, 0.02, (64, 6))
        src[37], tgt[37], states[37] = 0, 1, st
        got = _bytes(eng.evaluate_robust_pairs(src, tgt, states, 0, want_structs=True)["structs"])
        assert got[37] == first and got[36] != first
        assert alone() == first                                   # and behind a call that filled 64 histograms
        given = alone([0.004])
        deltas = rs.uniform(0.001, 0.01, 64)
        deltas[37] = 0.004
        got = _bytes(eng.evaluate_robust_pairs(src, tgt, states, 0, deltas=deltas, want_structs=True)["structs"])
        assert got[37] == given and given != first
        # the settings DESIGN.md §20 calls "accepted, no effect"
        for setter, values in ((eng.set_level_fusion, [native.FUSION_OFF, native.FUSION_AUTO]), (eng.set_wide_policy, [1, 0]),
                               (eng.set_latency_forms, [True, False]), (eng.set_batch_invariant, [True, False]),
                               (eng.set_slide_policy, [-1, 0])):
            for v in values:
                setter(v)
                assert alone() == first, (setter.__name__, v)
        eng.enqueue_align([0, 2] * 32, [1, 3] * 32)                 # an enqueue in flight before the call
        assert alone() == first
        eng.fetch_results(64)


def test_bit_identical_across_a_group_boundary():
    """4030 pairs of 8x8: one more than a group by the host's own formula (64 MiB / (256 B of tile sums + 16 KiB of histogram
    + 16 B) = 4029).  Pairs 0, 4028 and 4029 -- the first and the last of the first group and the only one of the second --
    have their own frames and state; the second group's histogram region is the first group's, cleared in between."""
    seq = cs.boundary_frames()
    n = cs.GROUP_PAIRS_8X8 + 1
    assert n == 4030
    src, tgt, states = np.zeros(n, dtype=int), np.ones(n, dtype=int), np.tile(cs.BOUNDARY_STATE, (n, 1))
    for q, (a, b, x) in cs.BOUNDARY_OWN.items():
        src[q], tgt[q], states[q] = a, b, x
    with _engine(seq["K"], 8, 8, frames=cs.BOUNDARY_FRAMES) as eng:
        eng.upload_frames(0, seq["gray"], seq["depth"])

        def alone(a, b, x):
            r = eng.evaluate_robust_pairs([a], [b], x[None], 0, want_structs=True)
            assert r["rows"][0] >= 32 and r["flags"][0] == 0 and r["delta"][0] > 0
            return _bytes(r["structs"])[0]
        one = alone(0, 1, cs.BOUNDARY_STATE)
        singles = {q: alone(*cs.BOUNDARY_OWN[q]) for q in cs.BOUNDARY_OWN}
        got = _bytes(eng.evaluate_robust_pairs(src, tgt, states, 0, want_structs=True)["structs"])
        deltas = np.full(n, 0.01)
        given_one = _bytes(eng.evaluate_robust_pairs([0], [1], cs.BOUNDARY_STATE[None], 0, deltas=[0.01], want_structs=True)["structs"])[0]
        deltas[cs.GROUP_PAIRS_8X8] = 0.02                        # the second group's delta is its own, not the first group's first
        a, b, x = cs.BOUNDARY_OWN[cs.GROUP_PAIRS_8X8]
        given_last = _bytes(eng.evaluate_robust_pairs([a], [b], x[None], 0, deltas=[0.02], want_structs=True)["structs"])[0]
        given = _bytes(eng.evaluate_robust_pairs(src, tgt, states, 0, deltas=deltas, want_structs=True)["structs"])
    assert len({one, *singles.values()}) == 4
    wrong = [q for q in range(n) if got[q] != singles.get(q, one)]
    assert not wrong, wrong[:10]
    assert given[1] == given_one and given[cs.GROUP_PAIRS_8X8] == given_last


# ---- no interference -----------------------------------------------------------------------------------------------------
def test_no_interference_with_alignments():
    import inverse_system_cases as ics
    seq = ics.four_frames()
    with _engine(seq["K"], ics.FOUR_W, ics.FOUR_H, frames=4, max_iter=[3]) as eng:
        eng.upload_frames(0, seq["gray"], seq["depth"])
        src, tgt = [0, 1, 2], [1, 2, 3]
        a0, r0 = eng.align_pairs(src, tgt, want_reports=True)
        rob0 = eng.fetch_robust_reports(3)
        eng.enqueue_align(src, tgt)
        ticket = eng.last_ticket()
        mid = eng.evaluate_robust_pairs(src, tgt, a0, 0)
        a1 = eng.fetch(ticket, 3)
        np.testing.assert_array_equal(a0, a1)
        a2, r2 = eng.fetch_results(3, want_reports=True)
        np.testing.assert_array_equal(a0, a2)
        assert _bytes(r0) == _bytes(r2)
        assert eng.fetch_robust_reports(3).tobytes() == rob0.tobytes()
        after = eng.evaluate_robust_pairs(src, tgt, a0, 0)
        for key in mid:
            np.testing.assert_array_equal(mid[key], after[key])
        assert mid["information"].shape == (3, 6, 6) and not mid["flags"].any()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _raw(eng, n, src, tgt, states, deltas, level, out):
    return eng._lib.phovo_engine_evaluate_robust_pairs(eng._h, n, src, tgt, states, deltas, level, out)


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except native.PhovoError as err:
        return err.status
    return 0


def test_refusals():
    p = cs.geometry_pair(75, 53)
    s, t = (C.c_int * 1)(0), (C.c_int * 1)(1)
    st = (C.c_double * 6)()
    d = (C.c_double * 1)(0.01)
    out = (native.RobustSystem * 1)()
    with _pair_engine(p, nl=2) as eng:
        assert _raw(eng, 1, s, t, st, None, 1, out) == native.OK and out[0].rows > 500
        assert _raw(eng, 1, s, t, st, d, 1, out) == native.OK and out[0].delta == 0.01 and out[0].median == 0.0
        assert _raw(eng, 0, None, None, None, None, 1, None) == native.OK
        for args in ((None, t, st, None, 1, out), (s, None, st, None, 1, out), (s, t, None, None, 1, out), (s, t, st, None, 1, None),
                     (None, t, st, d, 1, out), (s, t, st, d, 1, None)):
            assert _raw(eng, 1, *args) == native.E_INVALID_ARGUMENT
        assert _raw(eng, -1, s, t, st, None, 1, out) == native.E_INVALID_ARGUMENT
        assert _raw(eng, 1, s, t, st, None, 2, out) == native.E_INVALID_ARGUMENT
        assert _raw(eng, 1, s, t, st, None, -1, out) == native.E_INVALID_ARGUMENT
        bad = (C.c_int * 1)(2)
        assert _raw(eng, 1, bad, t, st, None, 1, out) == native.E_INVALID_ARGUMENT
        assert _raw(eng, 1, s, bad, st, None, 1, out) == native.E_INVALID_ARGUMENT
        # the five older calls stay refused under this objective, and name the new one
        zero6, zero8 = np.zeros((1, 6)), np.zeros((1, 8))
        assert _status(eng.evaluate_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_sampled_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert b"phovo_engine_evaluate_robust_pairs" in native.lib().phovo_last_error()
        assert _status(eng.evaluate_sampled_pairs, [0], [1], zero8, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_objective_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert b"phovo_engine_evaluate_robust_pairs" in native.lib().phovo_last_error()
        assert _status(eng.evaluate_geometric_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        assert _status(eng.evaluate_inverse_pairs, [0], [1], zero6, 0) == native.E_UNSUPPORTED
        # every other objective that keeps this frame pool
        for objective in (native.OBJECTIVE_PHOTOMETRIC, native.OBJECTIVE_PHOTOMETRIC_AFFINE,
                          native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC, INVERSE):
            eng.set_objective(objective)
            assert _raw(eng, 1, s, t, st, None, 1, out) == native.E_UNSUPPORTED
        eng.set_objective(ROBUST)
        assert _raw(eng, 1, s, t, st, None, 1, out) == native.OK
    for objective in (native.OBJECTIVE_BIOBJECTIVE, native.OBJECTIVE_TRUST_REGION):
        with odometry.AlignmentEngine() as eng:
            eng.set_config(native.make_config(num_levels=2, max_iter=[2, 2], min_grad=[0.0, 0.0]))
            eng.set_objective(objective)
            assert _status(eng.evaluate_robust_pairs, [0], [1], np.zeros((1, 6)), 0) == native.E_UNSUPPORTED
    with _engine(p["K"], 75, 53) as eng:                         # eval_check's order: arguments, frames, roles
        assert _status(eng.evaluate_robust_pairs, [0], [1], np.zeros((1, 6)), 0) == native.E_NOT_READY
        eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
        eng.upload_frame(1, p["gray1"], p["depth1"])
        assert _status(eng.evaluate_robust_pairs, [0], [1], np.zeros((1, 6)), 0) == native.E_NOT_READY
        assert b"gradient" in native.lib().phovo_last_error()
        assert _status(eng.evaluate_robust_pairs, [1], [1], np.zeros((1, 6)), 0) == native.OK
        eng.upload_frame(0, p["gray0"], p["depth0"])
        assert _status(eng.evaluate_robust_pairs, [0], [1], np.zeros((1, 6)), 0) == native.OK


# ---- the class surface ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter,finest", [([3, 4], 0), ([0, 4], 1)])
def test_class_surface_matches_engine(max_iter, finest):
    import inverse_system_cases as ics
    p = ics.levels_pair()
    cfg = native.make_config(num_levels=2, max_iter=max_iter, min_grad=[0.0] * 2)
    with odometry.CPhotoconsistencyOdometryRobust() as od:
        od.SetConfiguration(cfg)
        od.SetIntrinsicMatrix(p["K"])
        od.SetSourceFrame(p["gray0"], p["depth0"])
        od.SetTargetFrame(p["gray1"], p["depth1"])
        with pytest.raises(native.PhovoError) as ex:
            od.GetRobustSystem()
        assert ex.value.status == native.E_NOT_READY
        od.Optimize()
        rs = od.GetRobustSystem()
        state = od.GetOptimalStateVector()
        with odometry.AlignmentEngine() as eng:
            eng.set_config(cfg)
            eng.set_objective(ROBUST)
            eng.set_intrinsic_matrix(p["K"])
            eng.reserve_frames(2, ics.LEVELS_W, ics.LEVELS_H)
            eng.upload_frame(0, p["gray0"], p["depth0"])
            eng.upload_frame(1, p["gray1"], p["depth1"])
            ref = eng.evaluate_robust_pairs([0], [1], state[None], finest, want_structs=True)["structs"][0]
        assert rs.rows > 1000 and rs.flags == 0 and rs.delta > 0 and rs.median > 0
        assert bytes(memoryview(rs)) == bytes(memoryview(ref))
        for getter in (od.GetPairSystem, od.GetSampledSystem):    # the older calls stay refused
            with pytest.raises(native.PhovoError) as ex:
                getter()
            assert ex.value.status == native.E_UNSUPPORTED
        od.SetSourceFrame(p["gray0"], p["depth0"])
        with pytest.raises(native.PhovoError) as ex:
            od.GetRobustSystem()
        assert ex.value.status == native.E_NOT_READY
    with odometry.CPhotoconsistencyOdometryInverse() as od:      # any other objective
        od.SetConfiguration(cfg)
        rs = native.RobustSystem()
        assert od._lib.phovo_odometry_get_robust_system(od._h, C.byref(rs)) == native.E_UNSUPPORTED
