"""The robust inverse-compositional checker (tests/inverse_robust_ref.py) against itself, against np.median and against the
closed forms of the histogram's edges; the accuracy under occlusion the objective was built for (DESIGN.md §22's table); the
pre-checks that give the GPU parity tests their footing; and the new symbols, constants, class and app method.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry
from oracle import numpy_twin as twin

import inverse_ref as ir
import inverse_robust_cases as cases
import inverse_robust_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the median rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 64, 479, 480])
def test_loop_and_vectorised_median_agree(n):
    rs = np.random.RandomState(n)
    for spread in (1e-4, 0.02, 0.7, 3.0):
        r = rs.normal(0, spread, n)
        r[rs.randint(0, n)] = np.nan if n > 2 else r[0]
        assert rr.median_loop(r) == rr.median_vectorised(r)
    assert rr.median_loop([]) == 0.0 and rr.median_vectorised(np.zeros(0)) == 0.0


@pytest.mark.parametrize("seed", range(8))
def test_median_rule_is_within_one_bin_of_the_exact_median(seed):
    """A grouped-data median lies in the bin that holds the sample median (the lower of the two middle values for even n:
    half = (n + 1) // 2), so it is within one bin width of it, and np.median of an even sample within the distance of the
    two middle values more; on these samples (thousands of values under 1) that distance is far below a bin."""
    rs = np.random.RandomState(seed)
    n = int(rs.randint(2000, 20000))
    r = np.concatenate([rs.normal(0, 10.0 ** rs.uniform(-3, -1), n), rs.uniform(-0.9, 0.9, n // 5)])
    m = rr.median_vectorised(r)
    exact = float(np.median(np.abs(r)))
    print(f"n {r.size}: grouped {m:.9f}, np.median {exact:.9f}, difference {abs(m - exact) * 4096:.3f} bins")
    assert abs(m - exact) <= 2.0 ** -12


def test_bins_at_their_edges():
    r = np.array([0.0, -0.0, 1.0 / 4096, np.nextafter(1.0 / 4096, 0), 1.0 - 2.0 ** -53, 1.0, -1.0, 3.0, np.inf, -np.inf, np.nan,
                  4095.0 / 4096])
    assert rr.bins(r).tolist() == [0, 0, 1, 0, 4095, 4095, 4095, 4095, 4095, 4095, 4095, 4095]
    assert rr.bins(r).min() >= 0 and rr.bins(r).max() <= rr.NB - 1


@pytest.mark.parametrize("kind", cases.EDGE_KINDS)
def test_histogram_edges_have_their_closed_forms(kind):
    """The edge fixtures at zero motion: r = I1 - I0 exactly, so m and the outlier count are known in closed form."""
    (i0, d0, gx0, gy0), i1, expect = cases.edge_planes(kind)
    R, t = ir.eigen_rt(np.zeros(6))
    r, _, rows = ir.rows_vectorised((i0, d0, gx0, gy0, i1), 0, cases.EDGE_K, R, t)
    r = r[rows]
    if kind != "nan target":
        np.testing.assert_array_equal(r, (i1 - i0).reshape(-1)[rows])          # exact
    m = rr.median_vectorised(r)
    assert m == rr.median_loop(r)
    if expect is not None:
        assert m == expect[0]
        assert int((np.abs(r) > rr.DEFAULT_SCALE * m).sum()) == expect[1]
    else:
        assert np.isnan(r).sum() > r.size / 2 and rr.bins(r)[np.isnan(r)].min() == rr.NB - 1
        assert 4095.0 / 4096 < m < 1.0
    if kind == "odd":
        assert r.size == 479
    if kind == "nan depth":
        assert r.size == 0


# ---- accuracy --------------------------------------------------------------------------------------------------------------
def twin_pyramid(p, nl, scale=0.0625):
    """The checker's pyramid on the twin's: the source's gradient planes are the Scharr of its own intensity level."""
    pyr = twin.build_pyramids(p["gray0"], p["depth0"], p["gray1"], nl, [scale] * nl)
    return [(i0, d0) + tuple(twin.scharr(i0, scale)) + (i1,) for i0, d0, i1, _, _ in pyr]


def _cfg(nl, mi, mg):
    return dict(num_levels=nl, lam=[1.0] * nl, max_iter=list(mi), min_grad=list(mg), min_depth=0.3, max_depth=5.0)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_accuracy_under_occlusion(seed):
    """160x120, 3 levels x 10 iterations, lambda 1 (test_inverse_cpu's set-up), a textured rectangle painted into the target:
    the robust aligner stays within 1e-3 of the generator's motion without an occluder and with a tenth of the image
    occluded, where objective 5's checker on the same planes is at least 10 x worse.  The 25 % row is printed only
    (DESIGN.md §22 records it)."""
    cfg = _cfg(3, [10] * 3, [0.0] * 3)
    for f in (0.0, 0.1, 0.25):
        p = cases.occluded_pair(seed, f)
        pyr = twin_pyramid(p, 3)
        robust = rr.optimize(pyr, p["K"], cfg)
        plain = ir.optimize(pyr, p["K"], cfg)
        err = float(np.abs(robust["state"] - p["motion"]).max())
        err_plain = float(np.abs(plain["state"] - p["motion"]).max())
        print(f"seed {seed} occluded {f:4.2f}: robust {err:.3e}, objective 5 {err_plain:.3e} ({err_plain / err:.1f} x), "
              f"delta {robust['delta']}, outliers {robust['outliers']} of {robust['valid_pixels']}")
        if f == 0.0:
            assert err <= 1e-3
        if f == 0.1:
            assert err <= 1e-3
            assert err_plain >= 10 * err


# ---- the GPU fixtures' footing ---------------------------------------------------------------------------------------------
def _check_footing(name, ref, angle_free=True):
    print(f"{name}: cond {ref['cond']:.3e}, margin {ref['margin']:.3e}, bin margin {ref['bin_margin']:.3e} bins, "
          f"delta margin {ref['delta_margin']:.3e}, it {ref['iterations']}, rows {ref['valid_pixels']}, "
          f"outliers {ref['outliers']}, delta {ref['delta']}")
    assert ref["flags"] == 0
    assert ref["cond"] <= 1e5, "the flat pose bar assumes cond(H) <= 1e5"
    assert ref["margin"] > 1e-6, "too close to a gradient threshold"
    assert ref["bin_margin"] >= cases.BIN_MARGIN_FLOOR, "an |r| * 4096 sits on an integer: choose another seed"
    assert ref["delta_margin"] >= cases.DELTA_MARGIN_FLOOR, "an |r| sits on its delta: choose another seed"
    assert np.abs(ref["state"][3:]).max() < 0.5, "angle keep-out (atan2's first octant, as §20's parity fixtures)"


@pytest.mark.parametrize("name", list(cases.PARITY))
def test_parity_fixtures_keep_their_distances(name):
    make, nl, mi, mg = cases.PARITY[name]
    p = make()
    ref = rr.optimize(twin_pyramid(p, nl), p["K"], _cfg(nl, mi, mg))
    _check_footing(name, ref)
    if name == "160x120 occluded":
        assert np.abs(ref["state"] - p["motion"]).max() <= 1e-3
        assert min(ref["outliers"]) > 0


def test_queue_identity_and_scale_fixtures_keep_their_distances():
    for seed in cases.QUEUE_SEEDS:
        p = cases.small_pair(seed, 24, 20)
        _check_footing(f"queue seed {seed}", rr.optimize(twin_pyramid(p, 2), p["K"], _cfg(2, [5, 5], [0.0, 0.0])))
    mx, my, nl, mi, mg = cases.IDENTITY
    for make in (mx, my):
        p = make()
        _check_footing("identity", rr.optimize(twin_pyramid(p, nl), p["K"], _cfg(nl, mi, mg)))
    make, nl, mi, mg = cases.SCALE_PAIR
    p = make()
    pyr = twin_pyramid(p, nl)
    default = rr.optimize(pyr, p["K"], _cfg(nl, mi, mg))
    _check_footing("scale default", default)
    huge = rr.optimize(pyr, p["K"], _cfg(nl, mi, mg), scale_factor=1e6)
    plain = ir.optimize(pyr, p["K"], _cfg(nl, mi, mg))
    assert huge["outliers"] == [0] * nl                                    # every weight is 1: objective 5's system
    np.testing.assert_allclose(huge["state"], plain["state"], rtol=0, atol=1e-12)
    half = rr.optimize(pyr, p["K"], _cfg(nl, mi, mg), scale_factor=0.5)
    _check_footing("scale 0.5", half)
    bar = rr.pose_bar(default["cond"], default["state"])
    assert np.abs(half["state"] - default["state"]).max() > 1000 * bar     # the option reaches the weights


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_the_surface_is_there():
    assert native.OBJECTIVE_INVERSE_ROBUST == 6
    assert native.LAUNCH_KINDS[11] == "inverse_robust"
    L = native.lib()
    for name in ("phovo_robust_options_default", "phovo_engine_set_robust_options", "phovo_engine_get_robust_options",
                 "phovo_engine_fetch_robust_reports", "phovo_odometry_set_robust_options",
                 "phovo_odometry_get_robust_options", "phovo_odometry_get_robust_report"):
        assert hasattr(L, name), name
    assert issubclass(odometry.CPhotoconsistencyOdometryRobust, odometry.CPhotoconsistencyOdometryAnalytic)
    for method in ("SetRobustOptions", "GetRobustOptions", "GetRobustReport"):
        assert hasattr(odometry.CPhotoconsistencyOdometryRobust, method)
    header = open(os.path.join(ROOT, "include", "phovo_hip.h")).read()
    assert "#define PHOVO_OBJECTIVE_INVERSE_ROBUST 6" in header
    assert "PHOVO_LAUNCH_INVERSE_ROBUST = 11" in header
    assert "int phovo_engine_fetch_robust_reports(phovo_engine *e, int n_pairs, phovo_robust_report *reports);" in header
    assert "q < 4096.0 ? (int)q : 4095" in header and "(double)(half - before) / (double)h[k]) * 0x1p-12" in header
    for d in ("phovo", "shim"):
        assert os.path.exists(os.path.join(ROOT, "include", d, "CPhotoconsistencyOdometryRobust.h"))
    opt = native.make_robust_options()
    assert opt.scale_factor == 1.345 * 1.4826
    assert odometry.ROBUST_REPORT_DTYPE.itemsize == native.C.sizeof(native.RobustReport)


def test_options_are_validated_without_a_device():
    L = native.lib()
    assert L.phovo_robust_options_default(None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_set_robust_options(None, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_get_robust_report(None, None) == native.E_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def apps():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])
    return os.path.join(ROOT, "apps", "bin")


def test_the_apps_name_the_method(apps):
    for app in ("PhotoconsistencyVisualOdometry", "PhotoconsistencyFrameAlignment"):
        r = subprocess.run([os.path.join(apps, app)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "|robust|" in r.stdout and "|inverse|" in r.stdout


@pytest.mark.parametrize("flag,needle", [
    ("--information", "--information needs --method analytic"),
    ("--system", "--system needs bilinear sampling or --method affine"),
    ("--geometric-system", "--geometric-system needs --method geometric"),
    ("--objective-system", "--objective-system needs --method ceres or --method biobjective"),
    ("--inverse-system", "--inverse-system needs --method inverse"),
])
def test_the_system_flags_refuse_the_method(apps, tmp_path, flag, needle):
    r = subprocess.run([os.path.join(apps, "PhotoconsistencyVisualOdometry"), "cfg.yml", str(tmp_path), str(tmp_path / "t.txt"),
                        "--method", "robust", flag, "s.txt"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert needle in r.stderr
    assert not (tmp_path / "t.txt").exists()
