"""The two C++ apps with --method ceres (GPU), i.e. the C++ class phovo::Ceres::CPhotoconsistencyOdometryCeres and the
batched engine: on a synthetic TUM-format sequence the VisualOdometry app writes the same trajectory file, byte for
byte, in its loop mode (the C++ class) and in --batch, and its poses are the CPU checker's chained poses
(tests/trust_region_ref.py); the FrameAlignment app prints the checker's pose and one "Ceres Solver Report" line per
optimised level; a configuration file of the wrong kind and --information with ceres are refused."""
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import trust_region_ref as ref
from test_gpu_apps import K_FA, K_VO, _read_trajectory, _write_tum

import phovo_amd  # noqa: F401
from phovo_amd import distributed, native, se3, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
CERES4 = os.path.join(ROOT, "tests", "golden", "ceres", "config_4_level_optimization_ceres.yml")
ANALYTIC4 = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])


def _vo(tmp_path, cfg, name, extra):
    out = tmp_path / "out" / f"{name}.txt"
    return subprocess.run([os.path.join(BIN, "PhotoconsistencyVisualOdometry"), cfg, str(tmp_path), str(out)] + extra,
                          capture_output=True, text=True, timeout=600), out


def test_visual_odometry_app_ceres_loop_and_batch_match_the_checker(tmp_path):
    frames = _write_tum(tmp_path, 6, K_VO)
    r_loop, loop = _vo(tmp_path, CERES4, "loop", ["--method", "ceres"])
    assert r_loop.returncode == 0, r_loop.stderr
    r_batch, batch = _vo(tmp_path, CERES4, "batch", ["--batch", "--method", "ceres"])
    assert r_batch.returncode == 0, r_batch.stderr
    assert open(loop).read() == open(batch).read()
    # the loop prints the solver's line for each of the 4 levels of every pair
    assert len(re.findall(r"^Ceres Solver Report: Iterations: \d+, Initial cost: \S+, Final cost: \S+, "
                          r"Termination: (CONVERGENCE|NO_CONVERGENCE|FAILURE)$", r_loop.stdout, re.M)) == 4 * 5

    cfg, opt = native.read_trust_region_file(CERES4)
    ocfg = ref.oracle_config(cfg)
    states = []
    for t in range(1, len(frames)):
        d0 = frames[t - 1][2].astype(np.float64) * (1.0 / 5000.0)
        s, recs = ref.align(ocfg, K_VO, frames[t - 1][1], d0, frames[t][1], opt)
        for L, rec in recs.items():
            assert min(rec["margins"], default=1.0) > 1e-6, (t, L)
        states.append(s)
    expect = distributed.trajectory_from_states(np.array(states))
    lines = _read_trajectory(loop)
    assert len(lines) == len(frames) - 1
    for k in range(len(lines)):
        f = [float(v) for v in lines[k].split()]
        np.testing.assert_allclose(f[1:4], expect[k][:3, 3], atol=1e-9)
        np.testing.assert_allclose(f[4:8], se3.rotation_to_quaternion(expect[k][:3, :3]), atol=1e-9)


def test_visual_odometry_app_refusals(tmp_path):
    _write_tum(tmp_path, 2, K_VO)
    for cfg, method, word in ((ANALYTIC4, "ceres", "ceres"), (CERES4, "analytic", "analytic|biobjective"),
                              (CERES4, "biobjective", "analytic|biobjective")):
        for extra in ([], ["--batch"]):
            r, _ = _vo(tmp_path, cfg, "x", extra + ["--method", method])
            assert r.returncode != 0
            assert f"is not a configuration file for --method {word}" in r.stderr, r.stderr
    r, _ = _vo(tmp_path, CERES4, "x", ["--batch", "--method", "ceres", "--information", str(tmp_path / "i.txt")])
    assert r.returncode != 0 and "--information needs --method analytic" in r.stderr, r.stderr


def _pair_files(tmp_path):
    p = synthetic.make_pair(4, 640, 480, holes=0.01)
    for i in (0, 1):
        Image.fromarray(p[f"gray{i}"]).save(tmp_path / f"g{i}.png")
        Image.fromarray(np.rint(p[f"depth{i}"] * 1000.0).astype(np.uint16)).save(tmp_path / f"d{i}.png")
    return p, [str(tmp_path / n) for n in ("g0.png", "d0.png", "g1.png", "d1.png")]


def test_frame_alignment_app_ceres_prints_the_checkers_pose(tmp_path):
    p, files = _pair_files(tmp_path)
    cfg, opt = native.read_trust_region_file(CERES4)
    d0 = np.rint(p["depth0"] * 1000.0).astype(np.uint16).astype(np.float64) * (1.0 / 1000.0)
    es, recs = ref.align(ref.oracle_config(cfg), K_FA, p["gray0"], d0, p["gray1"], opt)
    r = subprocess.run([os.path.join(BIN, "PhotoconsistencyFrameAlignment"), CERES4] + files + ["--method", "ceres"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    reports = re.findall(r"^Ceres Solver Report: Iterations: (\d+), Initial cost: (\S+), Final cost: (\S+), "
                         r"Termination: (\S+)$", r.stdout, re.M)
    names = {ref.TR_MAX_ITERATIONS: "NO_CONVERGENCE", ref.TR_INVALID_STEP: "FAILURE", ref.TR_EVALUATION_FAILED: "FAILURE"}
    expect = [recs[L] for L in sorted(recs, reverse=True)]                  # coarse to fine
    assert len(reports) == len(expect)
    for (its, c0, c1, term), rec in zip(reports, expect):
        assert int(its) == rec["steps"] + 1
        assert abs(float(c0) - rec["initial_cost"]) <= 1e-5 * rec["initial_cost"]     # %e: 7 significant digits
        assert abs(float(c1) - rec["final_cost"]) <= 1e-5 * rec["final_cost"]
        assert term == names.get(rec["termination"], "CONVERGENCE")
    body = r.stdout.split("main::Rt eigen:")[1].strip().split("\n")[:4]
    Rt = np.array([[float(v) for v in row.split()] for row in body])
    np.testing.assert_allclose(Rt, se3.eigen_pose(es), atol=1e-5)    # default ostream precision: 6 digits


def test_frame_alignment_app_refuses_the_other_kind_of_file(tmp_path):
    _, files = _pair_files(tmp_path)
    for cfg, method in ((ANALYTIC4, "ceres"), (CERES4, "analytic")):
        r = subprocess.run([os.path.join(BIN, "PhotoconsistencyFrameAlignment"), cfg] + files + ["--method", method],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0
        assert "is not a configuration file for --method" in r.stderr, r.stderr
