"""PhotoconsistencyVisualOdometry --objective-system (GPU) on the synthetic TUM-format sequence of tests/test_gpu_apps.py,
under --method ceres and --method biobjective: the loop (class surface) and --batch (engine) write the same file byte for
byte, every line is the record phovo_engine_evaluate_objective_pairs gives for that pair at the trajectory's state, the
trajectory files do not change with the flag, and --method analytic is refused."""
import os
import subprocess

import pytest

from test_gpu_apps import K_VO, _write_tum

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
CFG_ANALYTIC = os.path.join(ROOT, "config_files", "config_5_level_optimization_analytic.yml")
CFG_CERES = os.path.join(ROOT, "tests", "golden", "ceres", "config_5_level_optimization_ceres.yml")
METHODS = {"ceres": (CFG_CERES, native.OBJECTIVE_TRUST_REGION), "biobjective": (CFG_ANALYTIC, native.OBJECTIVE_BIOBJECTIVE)}


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    d = tmp_path_factory.mktemp("tum")
    return d, _write_tum(d, 4, K_VO)


def _vo(d, cfg, name, extra, expect_ok=True):
    out = d / "out" / f"{name}.txt"
    r = subprocess.run([os.path.join(BIN, "PhotoconsistencyVisualOdometry"), cfg, str(d), str(out)] + extra,
                       capture_output=True, text=True, timeout=600)
    if not expect_ok:
        return r
    assert r.returncode == 0, r.stderr
    return open(out).read()


@pytest.mark.parametrize("method", list(METHODS))
def test_objective_system_file_loop_and_batch(sequence, tmp_path, method):
    d, frames = sequence
    cfg_file, objective = METHODS[method]
    flags = ["--method", method]
    sys_loop, sys_batch = tmp_path / "obj_loop.txt", tmp_path / "obj_batch.txt"
    traj_plain_batch = _vo(d, cfg_file, method + "_plain_batch", flags + ["--batch"])
    traj_loop = _vo(d, cfg_file, method + "_loop", flags + ["--objective-system", str(sys_loop)])
    traj_batch = _vo(d, cfg_file, method + "_batch", flags + ["--batch", "--objective-system", str(sys_batch)])
    assert traj_plain_batch == traj_batch and traj_loop == traj_batch
    loop_bytes, batch_bytes = sys_loop.read_bytes(), sys_batch.read_bytes()
    assert loop_bytes == batch_bytes
    lines = loop_bytes.decode().strip().split("\n")
    n = len(frames) - 1
    assert len(lines) == n

    # the same pairs through the engine: aligned from the zero state as the app does, evaluated at the returned states on
    # the finest level the file optimises
    if objective == native.OBJECTIVE_TRUST_REGION:
        ncfg, opt = native.read_trust_region_file(cfg_file)
    else:
        ncfg, opt = native.read_config_file(cfg_file), None
    finest = min(l for l in range(ncfg.num_levels) if ncfg.max_num_iterations[l] > 0)
    with odometry.AlignmentEngine() as eng:
        eng.set_config(ncfg)
        eng.set_objective(objective)
        if opt is not None:
            eng.set_trust_region_options(opt)
        eng.set_batch_invariant(True)
        eng.set_intrinsic_matrix(K_VO)
        eng.reserve_frames(len(frames), 640, 480)
        for i, (_, gray, d16) in enumerate(frames):
            eng.upload_frame(i, gray, d16.astype("float64") * (1.0 / 5000.0))
        src, tgt = list(range(n)), list(range(1, n + 1))
        states = eng.align_pairs(src, tgt)
        recs = eng.evaluate_objective_pairs(src, tgt, states, finest, want_structs=True)
    finest_pixels = (640 >> finest) * (480 >> finest)
    for p, ln in enumerate(lines):
        fields = ln.split()
        assert len(fields) == 3 + 21
        assert float(fields[0]) == float(f"{frames[p + 1][0]:.6f}")               # the timestamp as rgb.txt states it
        assert int(fields[1]) == recs["rows"][p] and finest_pixels // 2 < recs["rows"][p] <= finest_pixels
        assert float(fields[2]) == recs["cost"][p] and recs["flags"][p] == 0
        assert ln == native.format_pair_system(float(fields[0]), recs["structs"][p])


def test_objective_system_refusals(sequence, tmp_path):
    d, _ = sequence
    out = str(tmp_path / "x.txt")
    r = _vo(d, CFG_ANALYTIC, "refused", ["--method", "analytic", "--objective-system", out], expect_ok=False)
    assert r.returncode != 0 and "--objective-system needs --method ceres or --method biobjective" in r.stderr
    r = _vo(d, CFG_ANALYTIC, "refused", ["--method", "biobjective", "--batch", "--gpus", "2", "--objective-system", out],
            expect_ok=False)
    assert r.returncode != 0 and "--objective-system runs on one device" in r.stderr
    r = _vo(d, CFG_ANALYTIC, "refused", ["--method", "biobjective", "--information", out], expect_ok=False)
    assert r.returncode != 0 and "--information needs --method analytic" in r.stderr
