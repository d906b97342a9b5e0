"""PhotoconsistencyVisualOdometry --system (GPU) on the synthetic TUM-format sequence of tests/test_gpu_apps.py, under
--method affine and under an analytic yml with sampling_bilinear: 1 / jacobian_corrected: 1: the loop (class surface) and
--batch (engine) write the same system file byte for byte, every line parses to the method's dim, and the trajectory file
does not change with the flag."""
import os
import subprocess

import pytest

from test_gpu_apps import K_VO, _write_tum

import phovo_amd  # noqa: F401
from phovo_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
CFG5 = os.path.join(ROOT, "config_files", "config_5_level_optimization_analytic.yml")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    d = tmp_path_factory.mktemp("tum")
    return d, _write_tum(d, 6, K_VO)


def _vo(d, cfg, name, extra):
    out = d / "out" / f"{name}.txt"
    r = subprocess.run([os.path.join(BIN, "PhotoconsistencyVisualOdometry"), str(cfg), str(d), str(out)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return open(out).read()


@pytest.mark.parametrize("method", ["affine", "bilinear"])
def test_system_file_loop_and_batch(sequence, tmp_path, method):
    d, frames = sequence
    if method == "affine":
        cfg, flags, dim = CFG5, ["--method", "affine"], 8
    else:
        cfg, flags, dim = tmp_path / "bilinear.yml", [], 6
        cfg.write_text(open(CFG5).read() + "sampling_bilinear: 1\njacobian_corrected: 1\n")
    sys_loop, sys_batch = tmp_path / "sys_loop.txt", tmp_path / "sys_batch.txt"
    traj_plain_loop = _vo(d, cfg, method + "_plain_loop", flags)
    traj_plain_batch = _vo(d, cfg, method + "_plain_batch", flags + ["--batch"])
    traj_loop = _vo(d, cfg, method + "_loop", flags + ["--system", str(sys_loop)])
    traj_batch = _vo(d, cfg, method + "_batch", flags + ["--batch", "--system", str(sys_batch)])
    assert traj_plain_loop == traj_loop and traj_plain_batch == traj_batch and traj_loop == traj_batch
    if method == "bilinear":            # the extension keys reach the engines of --batch
        assert traj_batch != _vo(d, CFG5, "nearest_batch", ["--batch"])
    loop_bytes, batch_bytes = sys_loop.read_bytes(), sys_batch.read_bytes()
    assert loop_bytes == batch_bytes
    lines = loop_bytes.decode().strip().split("\n")
    ncfg = native.read_config_file(CFG5)
    finest = min(l for l in range(ncfg.num_levels) if ncfg.max_num_iterations[l] > 0)
    finest_pixels = (640 >> finest) * (480 >> finest)
    assert len(lines) == len(frames) - 1
    for p, ln in enumerate(lines):
        f = ln.split()
        assert len(f) == 4 + dim * (dim + 1) // 2 and int(f[3]) == dim
        assert float(f[0]) == float(f"{frames[p + 1][0]:.6f}")                # the timestamp as rgb.txt states it
        # rows of the finest level the file optimises: a frame-to-frame motion of a few pixels and 1 % of depth holes leave
        # most of its pixels in the image -- more than half of them is a floor no healthy pair comes near
        assert finest_pixels // 2 < int(f[1]) <= finest_pixels and float(f[2]) > 0.0
        assert all(float(f[4 + k]) > 0.0 for k in (0, dim, 2 * dim - 1))     # H00, H11, H22
