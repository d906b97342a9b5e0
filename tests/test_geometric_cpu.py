"""The photometric-geometric checker (tests/geometric_ref.py) against itself, against the twin's bilinear-corrected rows it
is built on and against central differences; the yml reader of the two optional keys; the apps' argument refusals; and the
pre-check of every fixture tests/test_gpu_geometric.py hands to the device.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native
from oracle import numpy_twin as twin

import geometric_cases as gc
import geometric_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_case(seed, W=9, H=7, spread=1.0):
    """Random planes; source and target depths with gate rejects (too near, too far, NaN) and a motion large enough, for
    the image size, to push pixels out of bounds and into every clamp band.  The target depth is the source depth plus a
    few centimetres of noise, so a residual limit of 5 cm drops some rows and keeps others."""
    rs = np.random.RandomState(seed)
    K = np.array([[60.0, 0, (W - 1) / 2.0], [0, 55.0, (H - 1) / 2.0], [0, 0, 1]])
    d0 = rs.uniform(1.5, 2.0, (H, W))
    d1 = d0 + rs.uniform(-0.12, 0.12, (H, W))
    d0.reshape(-1)[rs.choice(W * H, 3, replace=False)] = [0.1, 7.0, np.nan]
    d1.reshape(-1)[rs.choice(W * H, 3, replace=False)] = [0.1, 7.0, np.nan]
    planes = (rs.uniform(0, 1, (H, W)), d0, rs.uniform(0, 1, (H, W)), rs.normal(0, 1, (H, W)), rs.normal(0, 1, (H, W)), d1)
    pose = np.concatenate([rs.uniform(-0.02, 0.02, 3) * spread, rs.uniform(-0.03, 0.03, 3) * spread])
    return planes, K, pose


def test_loop_and_vectorised_forms_agree_and_reach_every_branch():
    total = {k: 0 for k in gr.COUNTERS}
    for seed in range(12):
        planes, K, pose = tiny_case(seed, spread=1.0 + seed % 3)
        for limit in (0.0, 0.05):
            v = gr.rows_vectorised(planes, 0, K, pose, 1.7, limit)
            l = gr.rows_loop(planes, 0, K, pose, 1.7, limit)
            np.testing.assert_array_equal(v["rows"], l["rows"])
            np.testing.assert_array_equal(v["drows"], l["drows"])
            for key in ("rI", "rD", "JI", "JD"):
                np.testing.assert_allclose(v[key], l[key], rtol=0, atol=1e-12 * max(1.0, np.abs(l[key]).max()))
            assert v["gate_margin"] == pytest.approx(l["gate_margin"], rel=1e-9)
            assert v["cell_margin"] == pytest.approx(l["cell_margin"], rel=1e-6)
            for k in gr.COUNTERS:
                total[k] += l["stats"][k]
    print(total)
    assert all(total[k] > 0 for k in gr.COUNTERS), total      # every gate side, NaN, the residual gate, every clamp band


def test_photometric_rows_are_the_twins_bilinear_corrected_rows():
    for seed in range(4):
        planes, K, pose = tiny_case(100 + seed)
        v = gr.rows_vectorised(planes, 0, K, pose, 2.0, 0.05)
        res, J6 = twin.normal_equations_bilinear(planes[:5], 0, K, pose, corrected=True)
        np.testing.assert_array_equal(v["rI"], res)
        np.testing.assert_array_equal(v["JI"], J6)
        assert v["rows"].sum() > 8 and 0 < v["drows"].sum() < v["rows"].sum()


@pytest.mark.parametrize("sigma", [0.3, 1.0, 40.0])
def test_with_every_target_depth_invalid_the_system_is_the_photometric_one(sigma):
    for bad in (0.0, 7.0, np.nan):
        planes, K, pose = tiny_case(7)
        planes = planes[:5] + (np.full_like(planes[5], bad),)
        s = gr.system(planes, 0, K, pose, sigma, 0.05)
        res, J6 = twin.normal_equations_bilinear(planes[:5], 0, K, pose, corrected=True)
        assert s["depth_rows"] == 0 and s["depth_cost"] == 0.0 and s["rows"] > 8
        np.testing.assert_array_equal(s["H"], J6.T @ J6)
        np.testing.assert_array_equal(s["g"], J6.T @ res)


def test_both_jacobians_against_central_differences():
    """On rows whose (u, v) stay inside one tap cell under the step both residuals are smooth (bilinear in (u, v), and
    (u, v) and Z' smooth in the pose), so central differences apply.  Step h = 1e-6: the truncation error is
    h^2 |r'''| / 6 ~ 1e-12 x O(10..1000) (third derivatives grow with the focal length) and the rounding error
    eps |r| / h ~ 2e-10 x O(1); the bar is 1e-6 of the column's largest entry (entries are O(1..100)), two orders above
    both.  A wrong sign, a missing sigma or a missing -dZ'/dp term is an error of the order of the entries themselves:
    -dZ'/dz alone is sigma = 3."""
    W, H, sigma, h = 12, 9, 3.0, 1e-6
    rs = np.random.RandomState(3)
    K = np.array([[60.0, 0, 5.5], [0, 55.0, 4.0], [0, 0, 1]])
    d0 = rs.uniform(1.0, 3.0, (H, W))
    planes = (rs.uniform(0, 1, (H, W)), d0, rs.uniform(0, 1, (H, W)), rs.normal(0, 1, (H, W)), rs.normal(0, 1, (H, W)),
              d0 + rs.uniform(-0.2, 0.2, (H, W)))
    pose = np.array([0.004, -0.003, 0.005, 0.004, -0.003, 0.002])
    # the gradient planes GX1, GY1 must BE the derivative of I1's interpolant for dr_I/dpose = GX1 du + GY1 dv to hold: a
    # ramp (tests/test_affine_cpu.py); the depth row needs no such help, its gradient is the interpolant's own
    cc, rr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    a, b = 0.03, -0.02
    planes = (planes[0], planes[1], a * cc + b * rr + 0.4, np.full((H, W), a), np.full((H, W), b), planes[5])
    base = gr.rows_vectorised(planes, 0, K, pose, sigma, 0.0)
    checked = 0
    for j in range(6):
        e = np.zeros(6); e[j] = h
        up = gr.rows_vectorised(planes, 0, K, pose + e, sigma, 0.0)
        dn = gr.rows_vectorised(planes, 0, K, pose - e, sigma, 0.0)
        # rows of all three evaluations that are at least 1e-3 pixels inside their cell at the centre: a step of 1e-6 in
        # the pose moves (u, v) by less than 1e-4 pixels here, so they stay in it
        inner = base["drows"] & up["drows"] & dn["drows"] & _inside_cell(planes, K, pose, 1e-3)
        assert inner.sum() > 40
        checked += int(inner.sum())
        for r, J in (("rI", "JI"), ("rD", "JD")):
            fd = (up[r] - dn[r]) / (2 * h)
            bar = 1e-6 * max(1.0, np.abs(base[J][inner, j]).max())
            np.testing.assert_allclose(fd[inner], base[J][inner, j], rtol=0, atol=bar)
        if j == 2:      # what the bar is for: without the -dZ'/dp term column 2 is off by sigma on EVERY row
            fd = (up["rD"] - dn["rD"]) / (2 * h)
            assert np.abs(fd[inner] - (base["JD"][inner, 2] + sigma)).min() > 0.99 * sigma
    assert checked > 240


def _inside_cell(planes, K, pose, margin):
    """Rows whose u and v are at least `margin` pixels from an integer and whose taps are not clamped."""
    H, W = planes[0].shape
    R, _ = gr._rotation(pose)
    cc, rr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pz = planes[1].reshape(-1)
    P = R @ np.stack([(cc.reshape(-1) - K[0, 2]) * pz / K[0, 0], (rr.reshape(-1) - K[1, 2]) * pz / K[1, 1], pz]) + \
        np.asarray(pose[:3]).reshape(3, 1)
    u, v = P[0] * K[0, 0] / P[2] + K[0, 2], P[1] * K[1, 1] / P[2] + K[1, 2]
    ok = (np.abs(u - np.rint(u)) > margin) & (np.abs(v - np.rint(v)) > margin)
    return ok & (u > 0) & (u < W - 1) & (v > 0) & (v < H - 1)


def test_defaults_and_the_yml_reader(tmp_path):
    d = native.make_geometric_options()
    assert list(d.depth_weight) == [1.0] * native.MAX_LEVELS and list(d.max_depth_residual) == [0.1] * native.MAX_LEVELS
    shipped = native.read_geometric_file(gc.SHIPPED_4_LEVEL)                 # no such keys: the defaults
    assert list(shipped.depth_weight) == list(d.depth_weight) and list(shipped.max_depth_residual) == list(d.max_depth_residual)
    body = open(gc.SHIPPED_4_LEVEL).read()

    def read(extra):
        f = tmp_path / "c.yml"
        f.write_text(body + extra)
        try:
            return native.read_geometric_file(str(f))
        except native.PhovoError as err:
            return err.status
    o = read("depth_weight (at each level): [3, 2.5, 2, 1.5, 9]\nmax_depth_residual (at each level): [0.05, 0, -1, 0.2]\n")
    assert list(o.depth_weight[:6]) == [3.0, 2.5, 2.0, 1.5, 9.0, 1.0]       # longer than numOptimizationLevels: kept
    assert list(o.max_depth_residual[:5]) == [0.05, 0.0, -1.0, 0.2, 0.1]
    assert native.read_config_file(str(tmp_path / "c.yml")).num_levels == 4   # the analytic reader ignores the two keys
    o = read("depth_weight (at each level): [3, 3, 3, 3]\n")                  # one key alone
    assert list(o.depth_weight[:4]) == [3.0] * 4 and list(o.max_depth_residual[:4]) == [0.1] * 4
    for bad in ("depth_weight (at each level): [1, 1, 1]\n",                 # shorter than numOptimizationLevels
                "max_depth_residual (at each level): [0.1]\n",
                "depth_weight (at each level): [1, 0, 1, 1]\n", "depth_weight (at each level): [1, -2, 1, 1]\n",
                "depth_weight (at each level): [1, nan, 1, 1]\n", "depth_weight (at each level): [1, inf, 1, 1]\n",
                "depth_weight (at each level): [1, x, 1, 1]\n"):
        assert read(bad) == native.E_CONFIG, bad
    L = native.lib()
    assert L.phovo_geometric_read_file(None, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_geometric_options_default(None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_set_geometric_options(None, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_fetch_geometric_reports(None, 0, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_get_geometric_report(None, None) == native.E_INVALID_ARGUMENT
    try:
        native.read_geometric_file(str(tmp_path / "missing.yml"))
        assert False
    except native.PhovoError as err:
        assert err.status == native.E_IO


@pytest.fixture(scope="module")
def apps():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])
    return os.path.join(ROOT, "apps", "bin")


@pytest.mark.parametrize("extra,needle", [
    (["--method", "geometric", "--information", "i.txt"], "--information needs --method analytic"),
    (["--method", "geometric", "--system", "s.txt"], "--system needs bilinear sampling or --method affine"),
])
def test_visual_odometry_app_refusals(apps, tmp_path, extra, needle):
    r = subprocess.run([os.path.join(apps, "PhotoconsistencyVisualOdometry"), "cfg.yml", str(tmp_path),
                        str(tmp_path / "t.txt")] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert needle in r.stderr
    assert not (tmp_path / "t.txt").exists()


def test_the_apps_name_the_method(apps, tmp_path):
    for app in ("PhotoconsistencyVisualOdometry", "PhotoconsistencyFrameAlignment"):
        r = subprocess.run([os.path.join(apps, app)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "affine|geometric]" in r.stdout
    # a Ceres file is refused for --method geometric as for the other analytic-file methods
    ceres = [f for f in os.listdir(os.path.join(ROOT, "config_files")) if "ceres" in f]
    if ceres:
        r = subprocess.run([os.path.join(apps, "PhotoconsistencyVisualOdometry"), os.path.join(ROOT, "config_files", ceres[0]),
                            str(tmp_path), str(tmp_path / "t.txt"), "--method", "geometric"], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode != 0 and "is not a configuration file for --method" in r.stderr


@pytest.mark.parametrize("name", list(gc.CASES))
def test_gpu_fixture_is_well_posed_for_the_checker_alone(name):
    """What tests/test_gpu_geometric.py relies on, asserted here on the numpy twin's pyramids of the same inputs: cond(H)
    <= 1e5 (the flat 1e-9 bar applies), no gradient threshold and no residual gate within 1e-6 relative, no row within
    CELL_FLOOR pixels of a pixel centre.  The cases singular by construction (geometric_cases.SINGULAR: an exactly zero
    column or no row) must be exactly that -- no finite entry in the state -- and carry no pose bar."""
    case = gc.CASES[name]()
    ref = gr.optimize(gc.twin_pyramid(case), case["K"], gc.checker_cfg(case), case["init"])
    print(name, {k: ref[k] for k in ("iterations", "valid_pixels", "depth_rows", "flags", "cond", "margin", "gate_margin",
                                     "cell_margin", "noise_level")})
    assert ref["margin"] > 1e-6 and ref["gate_margin"] > 1e-6 and ref["cell_margin"] > gc.CELL_FLOOR
    assert ref["noise_level"] is None
    if name in gc.SINGULAR:
        assert ref["cond"] == np.inf and not np.any(np.isfinite(ref["state"])) and ref["flags"] & gr.PAIR_NONFINITE
    else:
        assert ref["cond"] <= 1e5 and ref["flags"] == 0 and np.all(np.isfinite(ref["state"]))
    gated = any(l > 0 for l, it in zip(case["limit"], case["mi"]) if it > 0)
    assert (ref["gate_margin"] < np.inf) == (gated and name != "all-invalid-target" and name != "all-nan-source")


@pytest.mark.parametrize("seed", gc.GROUND_TRUTH_SEEDS)
def test_ground_truth_seed_shows_a_factor_of_two_in_the_checker(seed):
    case = gc.ground_truth_case(seed)
    pyr = gc.twin_pyramid(case)
    geo = gr.optimize(pyr, case["K"], gc.checker_cfg(case))["state"]
    photo, _, _ = twin.optimize([q[:5] for q in pyr], case["K"],
                                dict(num_levels=case["nl"], lam=case["lam"], max_iter=case["mi"], min_grad=case["mg"],
                                     bilinear=True, corrected=True))
    m = case["pair"]["motion"]
    e_geo, e_photo = np.abs(geo - m).max(), np.abs(photo - m).max()
    print(f"seed {seed}: geometric {e_geo:.3e}, bilinear-corrected photometric {e_photo:.3e}, factor {e_photo / e_geo:.1f}")
    assert e_photo >= 2.0 * e_geo
