"""Both apps under --method semidense (GPU): PhotoconsistencyVisualOdometry on the synthetic TUM-format sequence of
tests/test_gpu_apps.py (four frames) -- the loop (class surface) and --batch (engine) write the same trajectory, which is the
Python engine's under the same thresholds, one value for all levels equals the same value given per level, the file's optional
key is read and the command line goes over it -- and PhotoconsistencyFrameAlignment against the Python class;
--min-pixel-gradient is refused without the method and with malformed values."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from test_gpu_apps import K_FA, K_VO, _read_trajectory, _write_tum

import phovo_amd  # noqa: F401
from phovo_amd import distributed, native, odometry, se3, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
CFG4 = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")
VO = os.path.join(BIN, "PhotoconsistencyVisualOdometry")
FA = os.path.join(BIN, "PhotoconsistencyFrameAlignment")
TAU = 0.06                                 # between the smallest and the largest gradient magnitude of the active levels


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    d = tmp_path_factory.mktemp("tum")
    return d, _write_tum(d, 4, K_VO)


def _vo(d, name, extra, ok=True, cfg=CFG4):
    out = d / "out" / f"{name}.txt"
    r = subprocess.run([VO, str(cfg), str(d), str(out)] + extra, capture_output=True, text=True, timeout=600)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    return _read_trajectory(out)


def test_visual_odometry_loop_batch_and_engine(sequence, tmp_path):
    d, frames = sequence
    flags = ["--method", "semidense"]
    loop = _vo(d, "loop", flags + ["--min-pixel-gradient", str(TAU)])
    batch = _vo(d, "batch", flags + ["--batch", "--min-pixel-gradient", str(TAU)])
    per_level = _vo(d, "per_level", flags + ["--batch", "--min-pixel-gradient", ",".join([str(TAU)] * 4)])
    dense = _vo(d, "dense", flags + ["--batch"])
    assert loop == batch == per_level and len(loop) == len(frames) - 1
    assert dense != batch
    # the file's optional key, and the command line over it
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(open(CFG4).read() + f"min_pixel_gradient (at each level): [ {TAU}, {TAU}, {TAU}, {TAU} ]\n")
    assert _vo(d, "from_file", flags, cfg=cfg) == loop
    assert _vo(d, "from_file_batch", flags + ["--batch"], cfg=cfg) == loop
    assert _vo(d, "over_file", flags + ["--batch", "--min-pixel-gradient", "0"], cfg=cfg) == dense
    # the engine under the same thresholds gives the poses the trajectory chains
    n = len(frames) - 1
    with odometry.AlignmentEngine() as eng:
        eng.read_configuration_file(CFG4)
        eng.set_objective(native.OBJECTIVE_INVERSE_SEMIDENSE)
        eng.set_semidense_options(native.make_semidense_options(TAU))
        eng.set_intrinsic_matrix(K_VO)
        eng.reserve_frames(len(frames), 640, 480)
        for f, (_, gray, d16) in enumerate(frames):
            eng.upload_frame(f, gray, d16.astype(np.float64) * (1.0 / 5000.0))
        states = eng.align_pairs(list(range(n)), list(range(1, n + 1)))
        sel = eng.fetch_semidense_reports(n)["selected"]
    # (the shipped file skips levels 0 and 1)
    assert np.all(sel[:, :2] == 0) and np.all((sel[:, 2] > 0) & (sel[:, 2] < 160 * 120)), sel
    expect = distributed.trajectory_from_states(states)
    for p in range(n):
        got = [float(v) for v in batch[p].split()]
        np.testing.assert_allclose(got[1:4], expect[p][:3, 3], atol=1e-12)
        np.testing.assert_allclose(got[4:8], se3.rotation_to_quaternion(expect[p][:3, :3]), atol=1e-12)


def test_frame_alignment_app(tmp_path):
    p = synthetic.make_pair(4, 640, 480, holes=0.01)
    for i in (0, 1):
        Image.fromarray(p[f"gray{i}"]).save(tmp_path / f"g{i}.png")
        Image.fromarray(np.rint(p[f"depth{i}"] * 1000.0).astype(np.uint16)).save(tmp_path / f"d{i}.png")
    files = [str(tmp_path / f) for f in ("g0.png", "d0.png", "g1.png", "d1.png")]
    r = subprocess.run([FA, CFG4] + files + ["--method", "semidense", "--min-pixel-gradient", f"{TAU},{TAU},{TAU},{TAU}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    body = r.stdout.split("main::Rt eigen:")[1].strip().split("\n")[:4]
    Rt = np.array([[float(v) for v in row.split()] for row in body])
    d0 = np.rint(p["depth0"] * 1000.0).astype(np.uint16).astype(np.float64) * (1.0 / 1000.0)
    d1 = np.rint(p["depth1"] * 1000.0).astype(np.uint16).astype(np.float64) * (1.0 / 1000.0)
    with odometry.CPhotoconsistencyOdometrySemiDense(0) as po:
        po.ReadConfigurationFile(CFG4)
        po.SetSemiDenseOptions(native.make_semidense_options(TAU))
        po.SetIntrinsicMatrix(K_FA)
        po.SetSourceFrame(p["gray0"], d0)
        po.SetTargetFrame(p["gray1"], d1)
        po.Optimize()
        state = po.GetOptimalStateVector()
        sel = list(po.GetSemiDenseReport().selected[:4])
    assert sel[:2] == [0, 0] and 0 < sel[2] < 160 * 120 and 0 < sel[3] < 80 * 60, sel      # (the file skips levels 0 and 1)
    np.testing.assert_allclose(Rt, se3.eigen_pose(state), atol=1e-5)    # default ostream precision: 6 digits


@pytest.mark.parametrize("method", [None, "analytic", "inverse", "robust"])
def test_the_flag_is_refused_without_the_method(sequence, tmp_path, method):
    d, _ = sequence
    flags = [] if method is None else ["--method", method]
    r = _vo(d, "refused", flags + ["--min-pixel-gradient", "0.1"], ok=False)
    assert r.returncode != 0 and "--min-pixel-gradient needs --method semidense" in r.stderr
    assert not (d / "out" / "refused.txt").exists()
    r = subprocess.run([FA, CFG4, "g0.png", "d0.png", "g1.png", "d1.png"] + flags + ["--min-pixel-gradient", "0.1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--min-pixel-gradient needs --method semidense" in r.stderr


@pytest.mark.parametrize("bad", ["-0.1", "nan", "inf", "0.1,", "0.1,x", "", "1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17"])
def test_malformed_values_are_refused(sequence, bad):
    d, _ = sequence
    r = _vo(d, "malformed", ["--method", "semidense", "--min-pixel-gradient", bad], ok=False)
    assert r.returncode != 0 and "--min-pixel-gradient" in r.stderr and "finite and >= 0" in r.stderr
    r = subprocess.run([FA, CFG4, "g0.png", "d0.png", "g1.png", "d1.png", "--method", "semidense", "--min-pixel-gradient", bad],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "finite and >= 0" in r.stderr
