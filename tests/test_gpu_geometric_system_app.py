"""PhotoconsistencyVisualOdometry --geometric-system (GPU) on the synthetic TUM-format sequence of tests/test_gpu_apps.py,
under --method geometric: the loop (class surface) and --batch (engine) write the same file byte for byte, every line parses
back to the record phovo_engine_evaluate_geometric_pairs gives for that pair at the trajectory's state, and the trajectory
files do not change with the flag."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_apps import K_VO, _write_tum

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

import geometric_system_ref as gsr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
CFG5 = os.path.join(ROOT, "config_files", "config_5_level_optimization_analytic.yml")
FLAGS = ["--method", "geometric"]


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    d = tmp_path_factory.mktemp("tum")
    return d, _write_tum(d, 6, K_VO)


def _vo(d, name, extra):
    out = d / "out" / f"{name}.txt"
    r = subprocess.run([os.path.join(BIN, "PhotoconsistencyVisualOdometry"), CFG5, str(d), str(out)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def test_geometric_system_file_loop_and_batch(sequence, tmp_path):
    d, frames = sequence
    sys_loop, sys_batch = tmp_path / "geo_loop.txt", tmp_path / "geo_batch.txt"
    traj_plain_loop = _vo(d, "plain_loop", FLAGS)
    traj_plain_batch = _vo(d, "plain_batch", FLAGS + ["--batch"])
    traj_loop = _vo(d, "loop", FLAGS + ["--geometric-system", str(sys_loop)])
    traj_batch = _vo(d, "batch", FLAGS + ["--batch", "--geometric-system", str(sys_batch)])
    assert traj_plain_loop == traj_loop and traj_plain_batch == traj_batch and traj_loop == traj_batch
    loop_bytes, batch_bytes = sys_loop.read_bytes(), sys_batch.read_bytes()
    assert loop_bytes == batch_bytes
    lines = loop_bytes.decode().strip().split("\n")
    assert len(lines) == len(frames) - 1

    # the same pairs through the engine: aligned from the zero state as the app does, evaluated at the returned states on
    # the finest level the file optimises
    ncfg = native.read_config_file(CFG5)
    finest = min(l for l in range(ncfg.num_levels) if ncfg.max_num_iterations[l] > 0)
    n = len(frames) - 1
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_objective(native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
        eng.set_geometric_options(native.read_geometric_file(CFG5))
        eng.set_intrinsic_matrix(K_VO)
        eng.reserve_frames(len(frames), 640, 480)
        for i, (_, gray, d16) in enumerate(frames):
            eng.upload_frame(i, gray, d16.astype(np.float64) * (1.0 / 5000.0))
        src, tgt = list(range(n)), list(range(1, n + 1))
        states = eng.align_pairs(src, tgt)
        recs = eng.evaluate_geometric_pairs(src, tgt, states, finest)
    finest_pixels = (640 >> finest) * (480 >> finest)
    for p, ln in enumerate(lines):
        rec = recs[p]
        got = gsr.parse_line(ln)
        assert got["timestamp"] == float(f"{frames[p + 1][0]:.6f}")              # the timestamp as rgb.txt states it
        assert finest_pixels // 2 < got["rows"] <= finest_pixels and 6 < got["depth_rows"] <= got["rows"]
        assert got["rows"] == rec["rows"] and got["depth_rows"] == rec["depth_rows"] and rec["flags"] == 0
        for name in ("photometric_cost", "depth_cost"):
            assert np.float64(got[name]).view(np.uint64) == rec[name].view(np.uint64), (p, name)
        for name in ("photometric_information", "depth_information", "information"):
            assert got[name].view(np.uint64).tolist() == rec[name].reshape(6, 6).view(np.uint64).tolist(), (p, name)
        assert ln == native.format_geometric_system(got["timestamp"], native.GeometricSystem.from_buffer_copy(rec.tobytes()))
