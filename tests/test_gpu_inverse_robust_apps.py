"""The VisualOdometry app with --method robust (GPU) on the small synthetic TUM-format sequence the other app tests build:
the same trajectory file, byte for byte, in its loop mode and in --batch, and not --method inverse's."""
import os
import subprocess

import pytest

from test_gpu_apps import K_VO, _write_tum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
CFG5 = os.path.join(ROOT, "config_files", "config_5_level_optimization_analytic.yml")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])


def _vo(tmp_path, name, extra):
    out = tmp_path / "out" / f"{name}.txt"
    r = subprocess.run([os.path.join(BIN, "PhotoconsistencyVisualOdometry"), CFG5, str(tmp_path), str(out)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def test_visual_odometry_app_robust_loop_and_batch_agree_byte_for_byte(tmp_path):
    frames = _write_tum(tmp_path, 12, K_VO)
    loop = _vo(tmp_path, "loop", ["--method", "robust"])
    batch = _vo(tmp_path, "batch", ["--batch", "--method", "robust"])
    assert loop == batch
    assert len(loop.strip().split("\n")) >= len(frames) - 1
    assert "nan" not in loop.lower()
    assert _vo(tmp_path, "inverse", ["--batch", "--method", "inverse"]) != batch            # the flag reaches the engine
