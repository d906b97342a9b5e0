"""phovo_engine_evaluate_robust_pairs / phovo_odometry_get_robust_system / phovo_robust_system_format without a device
(DESIGN.md §23): the symbols in the header, the binding and the library; the wrapper's argument checks; the checker
(tests/robust_system_ref.py) against its pixel-by-pixel form, and at unit weights against inverse_system_ref.system; the
order of the three costs; the format line; every fixture of tests/robust_system_cases.py held, on the oracle's CPU planes, to
what tests/test_gpu_robust_system.py relies on; the sweep's draws, their coverage, and that the checker alone sets aside none
of the committed seed's cases; and the reason the call exists, on the numpy model: at the robust optimum of an occluded pair
the weighted system's Newton step is the smaller one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry
from oracle import numpy_twin as twin

import inverse_edges as ie
import inverse_robust_edges as re_
import inverse_robust_ref as rr
import inverse_system_ref as isr
import inverse_system_sweep
import objective_system_sweep
import robust_system_cases as cs
import robust_system_ref as rsr
import robust_system_sweep as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phovo_engine_evaluate_robust_pairs", "phovo_odometry_get_robust_system", "phovo_robust_system_format")


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_the_three_symbols_stand_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "phovo_hip.h")).read()
    lib = C.CDLL(native.library_path())
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in native.SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct phovo_robust_system {" in header
    cpp = open(os.path.join(ROOT, "include", "phovo", "CPhotoconsistencyOdometryRobust.h")).read()
    assert "GetRobustSystem" in cpp
    assert "not built yet" not in header
    # the record is the header's, field by field
    assert C.sizeof(native.RobustSystem) == 36 * 8 + 6 * 8 + 5 * 8 + 4 * 4
    assert [f[0] for f in native.RobustSystem._fields_] == ["information", "gradient", "cost", "huber_cost", "squared_cost",
                                                            "delta", "median", "rows", "outliers", "flags", "reserved"]
    assert odometry.ROBUST_SYSTEM_DTYPE.itemsize == C.sizeof(native.RobustSystem)
    for name in odometry.ROBUST_SYSTEM_DTYPE.names:
        assert odometry.ROBUST_SYSTEM_DTYPE.fields[name][1] == getattr(native.RobustSystem, name).offset, name


def test_null_handles_are_refused_without_a_device():
    lib = native.lib()
    out = native.RobustSystem()
    assert lib.phovo_engine_evaluate_robust_pairs(None, 0, None, None, None, None, 0, None) == native.E_INVALID_ARGUMENT
    assert lib.phovo_odometry_get_robust_system(None, C.byref(out)) == native.E_INVALID_ARGUMENT
    buf = C.create_string_buffer(1024)
    assert lib.phovo_robust_system_format(0.0, None, buf, 1024) == native.E_INVALID_ARGUMENT
    assert lib.phovo_robust_system_format(0.0, C.byref(out), None, 1024) == native.E_INVALID_ARGUMENT


def test_wrapper_argument_checks():
    eng = odometry.AlignmentEngine.__new__(odometry.AlignmentEngine)          # no device: the checks come before the call
    with pytest.raises(ValueError):
        eng.evaluate_robust_pairs([0, 0], [1], np.zeros((2, 6)), 0)
    eng._lib, eng._h = native.lib(), None
    with pytest.raises(ValueError):
        eng.evaluate_robust_pairs([0], [1], np.zeros((1, 5)), 0)                # states are [n, 6]
    with pytest.raises(ValueError):
        eng.evaluate_robust_pairs([0], [1], np.zeros((1, 8)), 0)
    with pytest.raises(ValueError):
        eng.evaluate_robust_pairs([0], [1], np.zeros((1, 6)), 0, deltas=[0.1, 0.2])   # one delta per pair
    for bad in cs.BAD_DELTAS:
        with pytest.raises(ValueError):
            eng.evaluate_robust_pairs([0, 0], [1, 1], np.zeros((2, 6)), 0, deltas=[0.1, bad])
    assert callable(getattr(odometry.CPhotoconsistencyOdometryRobust, "GetRobustSystem"))
    for cls in (odometry.CPhotoconsistencyOdometryAnalytic, odometry.CPhotoconsistencyOdometryAffine,
                odometry.CPhotoconsistencyOdometryGeometric, odometry.CPhotoconsistencyOdometryCeres,
                odometry.CPhotoconsistencyOdometryInverse):
        assert not hasattr(cls, "GetRobustSystem")


def test_the_format_line_of_a_record():
    rs = native.RobustSystem()
    H = np.arange(36, dtype=np.float64).reshape(6, 6)
    H = H + H.T
    for i, v in enumerate(H.reshape(-1)):
        rs.information[i] = v
    for i in range(6):
        rs.gradient[i] = -0.5 * (i + 1)
    rs.cost, rs.huber_cost, rs.squared_cost, rs.delta, rs.median = 1.25, 1.5, 2.75, 0.1 / 3, 1.0 / 60
    rs.rows, rs.outliers, rs.flags = 4321, 123, 0
    line = native.format_robust_system(1311868164.363181, rs)
    f = line.split()          # timestamp rows outliers delta median cost huber_cost squared_cost, 6 of g, 21 of the triangle
    assert len(f) == 8 + 6 + 21 and float(f[0]) == 1311868164.363181 and f[1:3] == ["4321", "123"]
    assert [float(v) for v in f[3:8]] == [0.1 / 3, 1.0 / 60, 1.25, 1.5, 2.75]             # %.17g round-trips
    assert [float(v) for v in f[8:14]] == [-0.5 * (i + 1) for i in range(6)]
    assert [float(v) for v in f[14:]] == list(H[np.triu_indices(6)])
    buf = C.create_string_buffer(len(line) + 1)
    assert native.lib().phovo_robust_system_format(1311868164.363181, C.byref(rs), buf, len(line) + 1) == native.OK
    assert native.lib().phovo_robust_system_format(1311868164.363181, C.byref(rs), buf, len(line)) == native.E_INVALID_ARGUMENT


# ---- the checker ---------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert (a["rows"], a["outliers"], a["delta"], a["median"]) == (b["rows"], b["outliers"], b["delta"], b["median"])
    np.testing.assert_allclose(a["H"], b["H"], rtol=0, atol=1e-12 * max(1.0, np.abs(b["H"]).max()))
    np.testing.assert_allclose(a["g"], b["g"], rtol=0, atol=1e-12 * max(1.0, np.abs(b["g"]).max()))
    for c in rsr.COSTS:
        assert abs(a[c] - b[c]) <= 1e-12 * max(b[c], 1e-300), c


@pytest.mark.parametrize("w,h", [(8, 8), (7, 5), (45, 1), (1, 45)])
def test_the_vectorised_checker_equals_the_loop_form(w, h):
    p = cs.geometry_pair(w, h)
    planes = ie.oracle_pyramid(p, 1)[0]
    for st in cs.three_states(p):
        for scale in cs.SCALES:
            _same(rsr.system(planes, 0, p["K"], st, scale), rsr.system_loop(planes, 0, p["K"], st, scale))
        _same(rsr.system(planes, 0, p["K"], st, delta=0.01), rsr.system_loop(planes, 0, p["K"], st, delta=0.01))


def test_at_unit_weights_the_checker_is_inverse_system_refs():
    p = cs.geometry_pair(75, 53)
    planes = ie.oracle_pyramid(p, 1)[0]
    for st in cs.three_states(p):
        H, g, cost, rows = isr.system(planes, 0, p["K"], st)
        for ref in (rsr.system(planes, 0, p["K"], st, cs.UNIT_SCALE), rsr.system(planes, 0, p["K"], st, delta=cs.UNIT_DELTA)):
            assert ref["rows"] == rows and ref["outliers"] == 0
            assert np.array_equal(ref["H"], H) and np.array_equal(ref["g"], g) and ref["squared_cost"] == cost
            assert ref["cost"] == ref["huber_cost"] == ref["squared_cost"]


def test_the_order_of_the_three_costs():
    p = cs.occluded_pair()
    planes = ie.oracle_pyramid(p, 1)[0]
    for st in cs.three_states(p):
        for scale in cs.SCALES:
            ref = rsr.system(planes, 0, p["K"], st, scale)
            assert ref["outliers"] > 0
            assert ref["cost"] < ref["huber_cost"] < ref["squared_cost"]         # w r^2 <= 2 rho(r) <= r^2, row by row
    for w, h in cs.GEOMETRIES:
        q = cs.geometry_pair(w, h)
        ref = rsr.system(ie.oracle_pyramid(q, 1)[0], 0, q["K"], np.zeros(6))
        assert ref["cost"] <= ref["squared_cost"] and ref["huber_cost"] <= ref["squared_cost"]


# ---- the fixtures --------------------------------------------------------------------------------------------------------
def _held(name, planes, level, K, state, scale=rr.DEFAULT_SCALE, well_posed=True, delta=None):
    ref = rsr.system(planes, level, K, state, scale, delta=delta)
    H = ref["H"]
    cond = np.linalg.cond(H) if np.all(np.isfinite(H)) and H.any() else np.inf
    print(f"{name}: rows {ref['rows']} outliers {ref['outliers']} delta {ref['delta']:.6g} cond {cond:.3g} "
          f"bin margin {ref['bin_margin']:.3g} delta margin {ref['delta_margin']:.3g}")
    assert rsr.margins_hold(ref), (name, ref["bin_margin"], ref["delta_margin"])
    if well_posed:
        assert ref["rows"] >= 6 and cond <= cs.COND_BAR, (name, ref["rows"], cond)
    return ref


@pytest.mark.parametrize("w,h", cs.GEOMETRIES, ids=["%dx%d" % s for s in cs.GEOMETRIES])
def test_fixture_tile_geometries(w, h):
    p = cs.geometry_pair(w, h)
    planes = ie.oracle_pyramid(p, 1)[0]
    for k, st in enumerate(cs.three_states(p)):
        _held(f"{w}x{h} state {k}", planes, 0, p["K"], st, well_posed=cs.well_posed_size(w, h))


def test_fixture_vga_and_the_occluded_pair():
    p = cs.vga_pair()
    ref = _held("640x480", ie.oracle_pyramid(p, 1)[0], 0, p["K"], p["motion"])
    assert ref["rows"] > 250000
    q = cs.occluded_pair()
    planes = ie.oracle_pyramid(q, 1)[0]
    for k, st in enumerate(cs.three_states(q)):
        ref = _held(f"160x120 occluded state {k}", planes, 0, q["K"], st)
        assert ref["outliers"] > 0.05 * ref["rows"]


def test_fixture_scale_factors_and_given_deltas():
    p = cs.geometry_pair(75, 53)
    planes = ie.oracle_pyramid(p, 1)[0]
    for k, st in enumerate(cs.three_states(p)):
        refs = [_held(f"75x53 state {k} scale {s}", planes, 0, p["K"], st, s) for s in cs.SCALES]
        assert refs[1]["delta"] < refs[2]["delta"] < refs[0]["delta"] and refs[1]["outliers"] > refs[0]["outliers"]
        unit = _held(f"75x53 state {k} unit", planes, 0, p["K"], st, cs.UNIT_SCALE)
        assert unit["outliers"] == 0
        small = _held(f"75x53 state {k} small delta", planes, 0, p["K"], st, delta=cs.SMALL_DELTA_SHARE * refs[0]["median"])
        assert small["outliers"] > 0.5 * small["rows"] and small["cost"] < small["squared_cost"]


@pytest.mark.parametrize("name", re_.PLACED_NAMES)
def test_fixture_placed_medians_across_three_tiles(name):
    planes, per_tile = cs.tiles_planes(name)
    placement = cs.tiles_placement(name)
    bins_ = {k for k, _ in placement}
    assert per_tile == [bins_] * 3                                # every bin's rows arrive from all three tiles
    d0 = planes[1].reshape(-1)
    n = sum(c for _, c in placement)
    assert [int(np.isfinite(d0[1024 * t:1024 * (t + 1)]).sum()) for t in range(3)] == [n // 3] * 3 and n <= 2880
    for scale in re_.PLACED_SCALES:
        rows, delta, outliers = re_.placed_expect(placement, scale)
        ref = rsr.system(planes, 0, cs.TILES_K, np.zeros(6), scale)
        assert (ref["rows"], ref["delta"], ref["outliers"]) == (rows, delta, outliers) and rows == n
        # six times the counts leave the median where inverse_robust_edges put it, up to the odd n's half
        assert abs(delta - re_.placed_expect(re_.PLACED[name], scale)[1]) <= scale * 2.0 ** -12


def test_fixture_first_step():
    for i, p in enumerate(cs.step_pairs()):
        planes = ie.oracle_pyramid(p, 1)[0]
        for st in (np.zeros(6), cs.STEP_START):
            _held(f"step pair {i}", planes, 0, p["K"], st)


@pytest.mark.parametrize("layout,count,const", cs.ROWS_CASES)
def test_fixture_small_systems(layout, count, const):
    K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
    ref = _held(f"{layout} {count} const {const}", planes, 0, K, np.zeros(6), well_posed=False)
    assert ref["rows"] == count
    if const:
        assert not ref["H"].any() and not ref["g"].any()
    assert rsr.flags_of(ref) == (rsr.PAIR_RANK_DEFICIENT if count < 6 else 0)


def test_fixture_nan_planes():
    p = cs.geometry_pair(75, 53)
    planes = ie.oracle_pyramid(p, 1)[0]
    st = p["motion"] + cs.NAN_SHIFT
    clean = _held("nan planes", planes, 0, p["K"], st)
    bad = rsr.system(cs.nan_gx_planes(planes), 0, p["K"], st)
    for key in ("rows", "delta", "median", "outliers") + rsr.COSTS:
        assert bad[key] == clean[key], key
    assert rsr.flags_of(bad) == rsr.PAIR_NONFINITE and rsr.flags_of(clean) == 0
    hit = isr.sampled_target_pixels(planes, 0, p["K"], st)
    nan_i1 = rsr.system(cs.nan_i1_planes(planes, hit), 0, p["K"], st)
    assert nan_i1["rows"] == clean["rows"] and nan_i1["last_bin"] > clean["last_bin"]       # NaN residuals: the last bin
    assert rsr.flags_of(nan_i1) == rsr.PAIR_NONFINITE and not np.isfinite(nan_i1["squared_cost"])
    assert rsr.margins_hold(nan_i1)
    empty = rsr.system((planes[0], np.full_like(planes[1], np.nan)) + planes[2:], 0, p["K"], st)
    assert (empty["rows"], empty["delta"], empty["median"], empty["cost"]) == (0, 0.0, 0.0, 0.0)
    assert rsr.flags_of(empty) == rsr.PAIR_RANK_DEFICIENT


def test_fixture_group_boundary():
    assert cs.GROUP_PAIRS_8X8 == 4029 and sorted(cs.BOUNDARY_OWN) == [0, 4028, 4029]
    seq = cs.boundary_frames()
    for q, (a, b, st) in list(cs.BOUNDARY_OWN.items()) + [(-1, (0, 1, cs.BOUNDARY_STATE))]:
        planes = ie.oracle_pyramid(cs.pair_of_frames(seq, a, b), 1)[0]
        ref = _held(f"boundary pair {q}", planes, 0, seq["K"], st, well_posed=False)
        assert ref["rows"] >= 32


# ---- the sweep -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return sw.draw_cases()


def test_sweep_draws_and_coverage(cases):
    assert len(cases) == sw.CASES == 200
    assert sw.SET_ASIDE_CAP == objective_system_sweep.SET_ASIDE_CAP == 0.02
    base = inverse_system_sweep.draw_cases()                      # the draws underneath are that sweep's, bit for bit
    for c, b in zip(cases, base):
        assert np.array_equal(c["states"], b["states"]) and np.array_equal(c["gray"], b["gray"]) and c["orders"] == b["orders"]
    assert sum(len(c["states"]) for c in cases) == 1174
    seen = sw.classes_seen(cases)
    print(seen)
    assert seen["scale"] == sorted(cs.SCALES) and seen["given"] == [False, True]
    assert seen["pairs"] == [1, 3, 40] and seen["orders"] == sorted(inverse_system_sweep.ORDERS)
    given = sum(c["given"] for c in cases)
    assert 0.2 * len(cases) <= given <= 0.4 * len(cases), given


def test_the_checker_alone_sets_no_more_of_the_seed_aside_than_the_cap(cases):
    aside, no_rows, smallest = [], 0, [np.inf, np.inf]
    for ci, c in enumerate(cases):
        refs, deltas, why = sw.references(c, sw.oracle_planes(c))
        assert deltas is None or (np.all(np.isfinite(deltas)) and np.all(deltas > 0))
        no_rows += sum(r["rows"] == 0 for r in refs)
        smallest = [min([smallest[0]] + [r["bin_margin"] for r in refs]), min([smallest[1]] + [r["delta_margin"] for r in refs])]
        if why:
            aside.append((ci, why))
    print("set aside", aside, "states without rows", no_rows, f"smallest margins {smallest[0]:.3g} bins, {smallest[1]:.3g}")
    assert len(aside) <= sw.SET_ASIDE_CAP * len(cases), aside


# ---- why the call exists ---------------------------------------------------------------------------------------------
def twin_pyramid(p, nl, scale=0.0625):
    """The checker's pyramid on the twin's (tests/test_inverse_robust_cpu.py's): the source's gradient planes are the Scharr
    of its own intensity level."""
    pyr = twin.build_pyramids(p["gray0"], p["depth0"], p["gray1"], nl, [scale] * nl)
    return [(i0, d0) + tuple(twin.scharr(i0, scale)) + (i1,) for i0, d0, i1, _, _ in pyr]


def _cfg(nl, mi, mg):
    return dict(num_levels=nl, lam=[1.0] * nl, max_iter=list(mi), min_grad=list(mg), min_depth=0.3, max_depth=5.0)


def test_at_the_robust_optimum_the_weighted_newton_step_is_the_smaller():
    """DESIGN.md §22's occluded fixture (seed 5, 160x120, a tenth of the target occluded) at the robust checker's optimum:
    the Newton step ||H^-1 g|| of the weighted system (this call's) against that of objective 5's unweighted system
    (DESIGN.md §21), which is not stationary there.  Only the order is asserted; §23 records both."""
    p = cs.occluded_pair()
    pyr = twin_pyramid(p, 3)
    state = rr.optimize(pyr, p["K"], _cfg(3, [10] * 3, [0.0] * 3))["state"]
    weighted = rsr.system(pyr[0], 0, p["K"], state)
    H, g, _, rows = isr.system(pyr[0], 0, p["K"], state)
    step_w = float(np.linalg.norm(np.linalg.solve(weighted["H"], weighted["g"])))
    step_u = float(np.linalg.norm(np.linalg.solve(H, g)))
    print(f"Newton step at the robust optimum: weighted {step_w:.3e}, unweighted {step_u:.3e} ({step_u / step_w:.1f} x); "
          f"rows {rows}, outliers {weighted['outliers']}, delta {weighted['delta']:.6g}")
    assert weighted["rows"] == rows and step_w < step_u
