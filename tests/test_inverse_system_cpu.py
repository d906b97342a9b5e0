"""phovo_engine_evaluate_inverse_pairs / phovo_odometry_get_inverse_system without a device: the symbols in
the header, the binding and the library; the wrapper's argument checks; the checker (tests/inverse_system_ref.py) against its
pixel-by-pixel form and against inverse_ref.system; the format line; every fixture of tests/inverse_system_cases.py held, on
the oracle's CPU planes, to what tests/test_gpu_inverse_system.py relies on; the sweep's draws, their coverage, and that the
checker alone sets aside none of the committed seed's cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

import inverse_edges as ie
import inverse_ref as ir
import inverse_system_cases as cs
import inverse_system_ref as isr
import inverse_system_sweep as sw
import objective_system_sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phovo_engine_evaluate_inverse_pairs", "phovo_odometry_get_inverse_system")


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_both_symbols_stand_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "phovo_hip.h")).read()
    lib = C.CDLL(native.library_path())
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in native.SYMBOLS, name
        assert hasattr(lib, name), name
    cpp = open(os.path.join(ROOT, "include", "phovo", "CPhotoconsistencyOdometryInverse.h")).read()
    assert "GetInverseSystem" in cpp
    # the contract states the perturbation in words
    assert "T(xi) = T Exp(xi)" in header and "SOURCE camera's frame" in header and "Ad_T" in header


def test_null_handles_are_refused_without_a_device():
    lib = native.lib()
    out = native.PairSystem()
    assert lib.phovo_engine_evaluate_inverse_pairs(None, 0, None, None, None, 0, None) == native.E_INVALID_ARGUMENT
    assert lib.phovo_odometry_get_inverse_system(None, C.byref(out)) == native.E_INVALID_ARGUMENT


def test_wrapper_argument_checks():
    eng = odometry.AlignmentEngine.__new__(odometry.AlignmentEngine)          # no device: the checks come before the call
    with pytest.raises(ValueError):
        eng.evaluate_inverse_pairs([0, 0], [1], np.zeros((2, 6)), 0)
    eng._lib, eng._h = native.lib(), None
    with pytest.raises(ValueError):
        eng.evaluate_inverse_pairs([0], [1], np.zeros((1, 5)), 0)               # states are [n, 6]
    with pytest.raises(ValueError):
        eng.evaluate_inverse_pairs([0], [1], np.zeros((1, 8)), 0)
    assert callable(getattr(odometry.CPhotoconsistencyOdometryInverse, "GetInverseSystem"))
    for cls in (odometry.CPhotoconsistencyOdometryAnalytic, odometry.CPhotoconsistencyOdometryAffine,
                odometry.CPhotoconsistencyOdometryGeometric, odometry.CPhotoconsistencyOdometryCeres):
        assert not hasattr(cls, "GetInverseSystem")
    assert "every Get...System()" not in odometry.CPhotoconsistencyOdometryInverse.__doc__


def test_the_format_line_of_a_record():
    ps = native.PairSystem()
    H = np.arange(36, dtype=np.float64).reshape(6, 6)
    H = H + H.T
    for i, v in enumerate(H.reshape(-1)):
        ps.information[i] = v
    for i in range(6):
        ps.gradient[i] = -0.5 * (i + 1)
    ps.cost, ps.rows, ps.flags = 1.25, 4321, 0
    line = native.format_pair_system(1311868164.363181, ps)
    fields = line.split()                                        # timestamp, rows, cost, the 21 entries of the upper triangle
    assert len(fields) == 24 and float(fields[0]) == 1311868164.363181 and fields[1] == "4321" and float(fields[2]) == 1.25
    assert [float(f) for f in fields[3:]] == list(H[np.triu_indices(6)])


# ---- the checker ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(8, 8), (7, 5), (45, 1), (1, 45)])
def test_the_vectorised_checker_equals_the_loop_form(w, h):
    p = cs.geometry_pair(w, h)
    planes = ie.oracle_pyramid(p, 1)[0]
    for st in cs.three_states(p):
        H, g, cost, rows = isr.system(planes, 0, p["K"], st)
        Hl, gl, costl, rowsl = isr.system_loop(planes, 0, p["K"], st)
        assert rows == rowsl
        np.testing.assert_allclose(H, Hl, rtol=0, atol=1e-12 * max(1.0, np.abs(Hl).max()))
        np.testing.assert_allclose(g, gl, rtol=0, atol=1e-12 * max(1.0, np.abs(gl).max()))
        assert abs(cost - costl) <= 1e-12 * max(costl, 1e-300)


def test_the_checker_is_inverse_refs_system_at_the_same_pose():
    p = cs.geometry_pair(75, 53)
    planes = ie.oracle_pyramid(p, 1)[0]
    for st in cs.three_states(p):
        H, g, cost, rows = isr.system(planes, 0, p["K"], st)
        g2, H2, rows2 = ir.system(planes, 0, p["K"], *ir.eigen_rt(st))
        assert rows == rows2 and np.array_equal(H, H2) and np.array_equal(g, g2)
        assert cost > 0 and np.array_equal(H, H.T)


# ---- the fixtures --------------------------------------------------------------------------------------------------------
def _held(name, planes, level, K, state, well_posed=True, lo=0.3, hi=5.0):
    H, g, cost, rows = isr.system(planes, level, K, state, lo, hi)
    cond = np.linalg.cond(H) if np.all(np.isfinite(H)) and H.any() else np.inf
    print(f"{name}: rows {rows} cond {cond:.3g} cost {cost:.3g}")
    assert cost > cs.COST_FLOOR, (name, cost)
    if well_posed:
        assert rows >= 6 and cond <= cs.COND_BAR, (name, rows, cond)
    return H, g, cost, rows


@pytest.mark.parametrize("w,h", cs.GEOMETRIES, ids=["%dx%d" % s for s in cs.GEOMETRIES])
def test_fixture_tile_geometries(w, h):
    p = cs.geometry_pair(w, h)
    planes = ie.oracle_pyramid(p, 1)[0]
    for k, st in enumerate(cs.three_states(p)):
        _held(f"{w}x{h} state {k}", planes, 0, p["K"], st, cs.well_posed_size(w, h))


def test_fixture_vga():
    p = cs.vga_pair()
    planes = ie.oracle_pyramid(p, 1)[0]
    _, _, _, rows = _held("640x480", planes, 0, p["K"], p["motion"])
    assert rows > 250000


@pytest.mark.parametrize("w,h,shift,depth_range", cs.EXACT_CASES)
def test_fixture_exact_positions(w, h, shift, depth_range):
    K, planes, state = ie.exact_problem(w, h, shift, depth_range)
    _, _, _, rows = _held(f"exact {w}x{h} {shift}", planes, 0, K, state, True, *depth_range)
    assert rows == ie.exact_rows(planes[1], shift)


@pytest.mark.parametrize("w,h,shift", cs.K_CASES)
def test_fixture_intrinsics_and_the_row_mutant(w, h, shift):
    p, K = ie.intrinsics_problem(w, h, shift)
    planes = ie.oracle_pyramid(p, 1)[0]
    H, _, _, _ = _held(f"intrinsics {w}x{h} {shift}", planes, 0, K, ie.K_INIT)
    with ie.row_focal_mutant("fy_fx"):
        Hm, _, _, _ = isr.system(planes, 0, K, ie.K_INIT)
    assert np.abs(Hm - H).max() > 1e6 * 1e-10 * np.abs(H).max()


def test_fixture_levels_1_and_2():
    p = cs.levels_pair()
    pyr = ie.oracle_pyramid(p, 3)
    for level in (1, 2):
        for k, st in enumerate(cs.three_states(p)):
            _held(f"level {level} state {k}", pyr[level], level, p["K"], st)


def test_fixture_large_rotations():
    p = ie.angle_pair()
    planes = ie.oracle_pyramid(p, 1)[0]
    states = cs.angle_states()
    assert len(states) == 35 and np.all(np.isfinite(states))
    rows = [isr.system(planes, 0, p["K"], st)[3] for st in states]
    for k in range(3):
        _held(f"0.4 rad on axis {k}", planes, 0, p["K"], states[k])
    assert sum(r == 0 for r in rows) >= ie.ANGLE_LOST and sum(r >= 6 for r in rows) >= ie.ANGLE_FINITE


def test_fixture_first_step():
    for i, p in enumerate(cs.step_pairs()):
        planes = ie.oracle_pyramid(p, 1)[0]
        for st in (np.zeros(6), cs.STEP_START):
            _held(f"step pair {i}", planes, 0, p["K"], st)


@pytest.mark.parametrize("layout,count,const", cs.ROWS_CASES)
def test_fixture_small_systems(layout, count, const):
    K, planes = ie.rows_problem(ie.ROWS_SEED[layout], layout, count, constant_source=const)
    H, g, cost, rows = _held(f"{layout} {count} const {const}", planes, 0, K, np.zeros(6), well_posed=count >= 6 and not const)
    assert rows == count
    if const:
        assert not H.any() and not g.any()
    assert isr.flags_of(H, g, cost, rows) == (isr.PAIR_RANK_DEFICIENT if count < 6 else 0)


def test_fixture_nan_planes():
    p = cs.geometry_pair(75, 53)
    planes = ie.oracle_pyramid(p, 1)[0]
    st = p["motion"] + cs.NAN_SHIFT
    clean = _held("nan planes", planes, 0, p["K"], st)
    H, g, cost, rows = isr.system(cs.nan_gx_planes(planes), 0, p["K"], st)
    assert (rows, cost) == (clean[3], clean[2]) and np.isfinite(cost)
    assert isr.flags_of(H, g, cost, rows) == isr.PAIR_NONFINITE
    hit = isr.sampled_target_pixels(planes, 0, p["K"], st)
    assert 0 < (~hit).sum() < hit.size                            # some target pixels are read by no row
    i1 = planes[4].copy()
    i1[~hit] = np.nan
    again = isr.system(planes[:4] + (i1,), 0, p["K"], st)
    assert again[3] == clean[3] and np.array_equal(again[0], clean[0]) and np.array_equal(again[1], clean[1])
    assert again[2] == clean[2]


def test_fixture_frame_pairs_of_every_order():
    seq = cs.four_frames()
    states = cs.four_states()
    assert {a == b for a, b in cs.PAIRS_OF_FOUR} == {True, False} and any(b < a for a, b in cs.PAIRS_OF_FOUR)
    for (a, b), st in zip(cs.PAIRS_OF_FOUR, states):
        assert np.linalg.norm(st) >= cs.SELF_PAIR_KEEP_OUT
        planes = ie.oracle_pyramid(cs.pair_of_frames(seq, a, b), 1)[0]
        _held(f"frames ({a}, {b})", planes, 0, seq["K"], st)


def test_fixture_group_boundary():
    assert cs.GROUP_PAIRS == 873 and sorted(cs.BOUNDARY_OWN) == [0, 872, 873]


# ---- the sweep -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return sw.draw_cases()


def test_sweep_draws_and_coverage(cases):
    assert len(cases) == sw.CASES == 200
    assert sw.SET_ASIDE_CAP == objective_system_sweep.SET_ASIDE_CAP == 0.02
    seen = sw.classes_seen(cases)
    print(seen)
    assert seen["size"] == sorted(objective_system_sweep.SIZE_CLASSES)
    assert seen["kind"] == sorted(sw.DEPTH_KINDS)
    assert seen["changed"] == [False, True] and seen["pairs"] == [1, 3, 40]
    assert seen["orders"] == sorted(sw.ORDERS) and seen["edge"] and seen["perturbed"]
    assert all(1 <= c["w"] <= 64 and 1 <= c["h"] <= 48 for c in cases)
    n_states = sum(len(c["states"]) for c in cases)
    n_edge = sum(int(c["edge"].sum()) for c in cases)
    assert 0.05 * n_states <= n_edge <= 0.15 * n_states, (n_edge, n_states)
    for c in cases:                                               # self-pairs keep away from the identity
        for k, o in enumerate(c["orders"]):
            if o == "self":
                assert np.linalg.norm(c["states"][k]) >= cs.SELF_PAIR_KEEP_OUT


def test_the_checker_alone_sets_no_case_of_the_seed_aside(cases):
    knives = []
    for ci, c in enumerate(cases):
        _, knife = sw.references(c, sw.oracle_planes(c))
        if knife:
            knives.append(ci)
    assert knives == [], knives
