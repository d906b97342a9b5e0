"""CPU tests of the semi-dense inverse-compositional objective (PHOVO_OBJECTIVE_INVERSE_SEMIDENSE; no GPU
needed): the surface, the wrapper's and the yml reader's argument checks, the checker's two forms against each other, the
accuracy table of DESIGN.md §25, the pre-check of every GPU fixture on the CPU pyramids, and two mutants of the selection
rule that the fixtures written for them must see."""
import os

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, synthetic

import inverse_ref as ir
import semidense_cases as sc
import semidense_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")


def test_the_surface_is_there():
    assert native.OBJECTIVE_INVERSE_SEMIDENSE == 7
    assert native.LAUNCH_KINDS[14] == "inverse_semidense"
    L = native.lib()
    for name in ("phovo_semidense_options_default", "phovo_semidense_read_file", "phovo_engine_set_semidense_options",
                 "phovo_engine_get_semidense_options", "phovo_engine_fetch_semidense_reports",
                 "phovo_odometry_set_semidense_options", "phovo_odometry_get_semidense_options",
                 "phovo_odometry_get_semidense_report"):
        assert hasattr(L, name), name
    assert issubclass(odometry.CPhotoconsistencyOdometrySemiDense, odometry.CPhotoconsistencyOdometryAnalytic)
    for name in ("set_semidense_options", "get_semidense_options", "fetch_semidense_reports"):
        assert hasattr(odometry.AlignmentEngine, name)
    assert callable(odometry.semidense_thresholds)
    header = open(os.path.join(ROOT, "include", "phovo_hip.h")).read()
    assert "#define PHOVO_OBJECTIVE_INVERSE_SEMIDENSE 7" in header
    assert "PHOVO_LAUNCH_INVERSE_SEMIDENSE = 14" in header
    assert os.path.exists(os.path.join(CSRC, "gn_inverse_semidense_kernel.hip"))
    assert "gn_inverse_semidense_kernel" in open(os.path.join(CSRC, "Makefile")).read()
    opt = native.make_semidense_options()
    assert list(opt.min_pixel_gradient) == [0.0] * native.MAX_LEVELS
    opt = native.make_semidense_options([0.5, 0.25])
    assert list(opt.min_pixel_gradient[:3]) == [0.5, 0.25, 0.0]
    assert list(native.make_semidense_options(0.125).min_pixel_gradient) == [0.125] * native.MAX_LEVELS


@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan"), float("inf"), -float("inf")])
def test_the_wrapper_refuses_bad_thresholds(bad):
    with pytest.raises(ValueError):
        native.make_semidense_options(bad)
    with pytest.raises(ValueError):
        native.make_semidense_options([0.0, bad])
    assert L_status_null() == native.E_INVALID_ARGUMENT


def L_status_null():
    return native.lib().phovo_semidense_options_default(None)


def _yml(tmp_path, extra):
    src = open(os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")).read()
    path = tmp_path / "cfg.yml"
    path.write_text(src + extra)
    return str(path)


def test_the_yml_key_round_trips(tmp_path):
    absent = native.read_semidense_file(_yml(tmp_path, ""))
    assert list(absent.min_pixel_gradient) == [0.0] * native.MAX_LEVELS
    vals = [0.5, 0.25, 0.125, 1.5]
    got = native.read_semidense_file(_yml(tmp_path, "min_pixel_gradient (at each level): [ 0.5, 0.25, 0.125, 1.5 ]\n"))
    assert list(got.min_pixel_gradient[:4]) == vals and list(got.min_pixel_gradient[4:]) == [0.0] * (native.MAX_LEVELS - 4)
    # the other readers still take the file: the key is ignored by them
    cfg = native.read_config_file(_yml(tmp_path, "min_pixel_gradient (at each level): [ 0.5, 0.25, 0.125, 1.5 ]\n"))
    assert cfg.num_levels == 4
    for extra in ("min_pixel_gradient (at each level): [ 0.5, 0.25 ]\n",            # fewer than numOptimizationLevels
                  "min_pixel_gradient (at each level): [ 0.5, -0.25, 0.1, 0.1 ]\n",
                  "min_pixel_gradient (at each level): [ 0.5, .nan, 0.1, 0.1 ]\n",
                  "min_pixel_gradient (at each level): [ 0.5, .inf, 0.1, 0.1 ]\n",
                  "min_pixel_gradient (at each level): [ 0.5, x ]\n"):
        with pytest.raises(native.PhovoError) as err:
            native.read_semidense_file(_yml(tmp_path, extra))
        assert err.value.status == native.E_CONFIG, extra


@pytest.mark.parametrize("w,h", [(8, 8), (7, 5), (13, 9)])
def test_loop_and_vectorised_forms_agree(w, h):
    """The list walked record by record gives the rows of the vectorised checker on the masked planes, for a tau that
    keeps about half of the pixels; the list is the mask in raster order."""
    p = synthetic.make_pair(3, w, h, holes=0.1, trans=0.01, rot=0.005)
    planes = sc.inverse_pyramid(p, 1, any_size=True)[0]
    tau = sc.quantile_taus([planes], 0.5)[0]
    assert sr.threshold_gap(planes, tau) > sc.GAP_FLOOR
    R, t = ir.eigen_rt([0.01, -0.02, 0.015, 0.02, -0.01, 0.03])
    r1, J1, rows1, lst = sr.rows_loop(planes, 0, p["K"], R, t, tau)
    mp, n_sel = sr.masked(planes, tau)
    r2, J2, rows2 = ir.rows_vectorised(mp, 0, p["K"], R, t)
    mask = sr.select(planes, tau)
    assert len(lst) == n_sel == int(mask.sum()) and 0 < n_sel < w * h
    assert [rr * w + cc for cc, rr in lst] == np.flatnonzero(mask.reshape(-1)).tolist()
    assert rows1.tolist() == rows2.tolist() and rows1.sum() > 0
    assert np.abs(r1 - r2).max() <= 1e-13 and np.abs(J1 - J2).max() <= 1e-10 * max(1.0, np.abs(J2).max())


ACCURACY_SEEDS = (1, 2, 3, 4, 5)
ACCURACY_KEPT = (1.0, 0.5, 0.25, 0.1, 0.05)


def test_accuracy_at_a_quarter_of_the_rows():
    """160x120, 3 levels x 10 iterations, lambda 1, synthetic.make_pair seeds 1-5 on the twin's pyramids, each level keeping
    the given fraction of its depth-valid pixels by gradient magnitude: the largest pose error against the generator's
    motion.  At 1/4 kept the error is at most 1e-3 on all five seeds (DESIGN.md §25 has the table this prints)."""
    nl = 3
    c = sc.cfg([10] * nl)
    table = {}
    for seed in ACCURACY_SEEDS:
        p = synthetic.make_pair(seed, 160, 120)
        pyr = sc.inverse_pyramid(p, nl)
        for kept in ACCURACY_KEPT:
            ref = sr.optimize(pyr, p["K"], c, sc.quantile_taus(pyr, kept))
            assert ref["flags"] == 0
            table[(kept, seed)] = (float(np.abs(ref["state"] - p["motion"]).max()), ref["cond"])
    print("| kept | " + " | ".join(f"seed {s}" for s in ACCURACY_SEEDS) + " | worst cond(H) |")
    for kept in ACCURACY_KEPT:
        errs = [table[(kept, s)][0] for s in ACCURACY_SEEDS]
        print(f"| {kept:g} | " + " | ".join(f"{e:.1e}" for e in errs) + f" | {max(table[(kept, s)][1] for s in ACCURACY_SEEDS):.1e} |")
    for seed in ACCURACY_SEEDS:
        assert table[(0.25, seed)][0] <= 1e-3, (seed, table[(0.25, seed)])


# ---- the GPU fixtures, pre-checked on the CPU ------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", sc.PARITY_SIZES)
@pytest.mark.parametrize("fraction", sc.FRACTIONS)
def test_precheck_single_level(w, h, fraction):
    p = sc.parity_pair(w, h)
    pyr = sc.inverse_pyramid(p, 1, any_size=True)
    # the two strips have no gradient across: a column of the system is exactly zero and the pose is NaN on both sides
    # (and a tenth of 7 x 5 is 4 pixels: fewer than 6 rows, no pose -- the GPU file compares its first system's counts)
    sc.precheck(pyr, p["K"], sc.cfg([5]), sc.quantile_taus(pyr, fraction), healthy=sc.parity_is_healthy(w, h, fraction))


@pytest.mark.parametrize("yaw", [False, True])
@pytest.mark.parametrize("fraction", sc.FRACTIONS)
def test_precheck_three_levels(yaw, fraction):
    p, init = sc.carry_pair(yaw)
    pyr = sc.inverse_pyramid(p, 3)
    sc.precheck(pyr, p["K"], sc.cfg([10] * 3), sc.quantile_taus(pyr, fraction), init)


@pytest.mark.parametrize("layout", sc.SMALL_LAYOUTS)
def test_precheck_small_lists(layout):
    """The committed seed is the one the search over SMALL_SEARCH finds; 6 and 7 listed pixels keep their rows under the
    flat bar, 5 are rank deficient from the row count alone; the pixels sit where the layout says."""
    conds = [sc.small_worst_cond(s, layout) for s in sc.SMALL_SEARCH]
    assert int(np.argmin(conds)) == sc.SMALL_SEED[layout], (int(np.argmin(conds)), min(conds))
    picks = sc.small_picks(sc.SMALL_SEED[layout], layout)
    waves = {(k // 64) % 4 for k in picks}
    assert waves == ({2} if layout == "one_chunk" else {0, 1, 2, 3})
    for count in (6, 7):
        K, planes = sc.small_problem(layout, count)
        ref = sc.precheck([planes], K, sc.cfg([sc.SMALL_ITER]), [sc.TAU])
        assert ref["selected"] == [count] and ref["valid_pixels"] == [count]
    K, planes = sc.small_problem(layout, 5)
    ref = sc.precheck([planes], K, sc.cfg([1]), [sc.TAU], healthy=False)
    assert ref["selected"] == [5] and ref["valid_pixels"] == [5] and ref["flags"] & ir.PAIR_RANK_DEFICIENT


@pytest.mark.parametrize("count", sc.WALK_COUNTS)
def test_precheck_compact_walk(count):
    K, planes = sc.walk_problem(count)
    ref = sc.precheck([planes], K, sc.cfg([sc.WALK_ITER]), [sc.TAU])
    assert ref["selected"] == [count]
    mask = sr.select(planes, sc.TAU).reshape(-1)
    assert {(int(k) // 64) % 4 for k in np.flatnonzero(mask)} == {0}          # wave 0's chunks alone


@pytest.mark.parametrize("kind", sc.EDGE_KINDS)
def test_precheck_rule_edges(kind):
    K, planes, tau, expected = sc.edge_problem(kind)
    ref = sc.precheck([planes], K, sc.cfg([3]), [tau], exact_pixels=kind in ("at_tau", "below_tau"))
    assert ref["selected"] == [expected]
    mask = sr.select(planes, tau).reshape(-1)
    assert all(bool(mask[k]) == (kind == "at_tau") for k in sc.EDGE_PIXELS)


def test_precheck_stale_slab_pairs():
    pairs = sc.stale_pairs()
    nl = len(sc.STALE_ITER)
    pyrs = [sc.inverse_pyramid(p, nl) for p in pairs]
    tau = sc.quantile_taus(pyrs[0], 0.9)
    refs = [sc.precheck(pyr, pairs[0]["K"], sc.cfg(sc.STALE_ITER), tau) for pyr in pyrs]
    n = [sc.STALE_W * sc.STALE_H, sc.STALE_W * sc.STALE_H // 4]
    print([r["selected"] for r in refs])
    for L in range(nl):
        assert refs[0]["selected"][L] > 0.8 * n[L] and 6 <= refs[1]["selected"][L] < 0.2 * n[L]
    assert refs[1]["selected"][0] < 0.03 * n[0]


@pytest.mark.parametrize("rule", ["strict", "l1"])
def test_a_mutant_of_the_rule_ends_far_away(rule):
    """> for >=, and |gx| + |gy| for the squared magnitude: on the fixture written for it the mutant's pose is more than
    1000 bars from the contract's."""
    K, planes, tau = sc.mutant_problem(rule)
    c = sc.cfg([3])
    good = sc.precheck([planes], K, c, [tau], exact_pixels=rule == "strict")
    bad = sr.optimize([planes], K, c, [tau], rule=rule)
    assert good["selected"] != bad["selected"]
    ratio = np.abs(good["state"] - bad["state"]).max() / sr.pose_bar(good["cond"], good["state"])
    print(f"{rule}: selected {good['selected']} -> {bad['selected']}, {ratio:.3g} bars")
    assert ratio > 1000.0
