"""PhotoconsistencyVisualOdometry --information (GPU) on the synthetic TUM-format sequence of tests/test_gpu_apps.py: the
loop (class surface) and --batch (engine) write the same information file byte for byte, the trajectory file does not
change with the flag, and a line is phovo_pair_system_format of phovo_engine_evaluate_pairs at the pair's optimal state."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_apps import K_VO, _write_tum

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

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


def test_information_file_loop_batch_and_engine(tmp_path):
    frames = _write_tum(tmp_path, 12, K_VO)
    info_loop, info_batch = tmp_path / "info_loop.txt", tmp_path / "info_batch.txt"
    traj_plain = _vo(tmp_path, "plain", ["--batch"])
    traj_loop = _vo(tmp_path, "loop", ["--information", str(info_loop)])
    traj_batch = _vo(tmp_path, "batch", ["--batch", "--information", str(info_batch)])
    assert traj_plain == traj_loop == traj_batch
    loop_bytes, batch_bytes = info_loop.read_bytes(), info_batch.read_bytes()
    assert loop_bytes == batch_bytes
    lines = loop_bytes.decode().strip().split("\n")
    assert len(lines) == len(frames) - 1
    for ln in lines:
        assert len(ln.split()) == 3 + 21

    cfg = native.read_config_file(CFG5)
    finest = min(l for l in range(cfg.num_levels) if cfg.max_num_iterations[l] > 0)
    n = len(frames)
    with odometry.AlignmentEngine() as eng:
        eng.set_config(cfg)
        eng.set_batch_invariant(True)
        eng.set_intrinsic_matrix(K_VO)
        eng.reserve_frames(n, 640, 480)
        eng.upload_frames(0, np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames]), depth_scale=1.0 / 5000.0)
        src, tgt = list(range(n - 1)), list(range(1, n))
        states = eng.align_pairs(src, tgt)
        sys = eng.evaluate_pairs(src, tgt, states, finest, want_structs=True)
    for p in (0, 5, n - 2):
        ts = float(f"{frames[p + 1][0]:.6f}")                  # the timestamp as rgb.txt states it
        assert float(lines[p].split()[0]) == ts
        assert lines[p] == native.format_pair_system(ts, sys["structs"][p])
        vals = [float(v) for v in lines[p].split()]
        assert int(vals[1]) == sys["rows"][p] and vals[2] == sys["cost"][p]
        iu = np.triu_indices(6)
        np.testing.assert_array_equal(np.array(vals[3:]), sys["information"][p][iu])
