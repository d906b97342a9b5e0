"""CPU tests of the pair-system surface (no GPU needed): phovo_pair_system_format, the NULL-argument refusals of the new
entry points, and the VisualOdometry app's usage errors for --information."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system(seed):
    rs = np.random.RandomState(seed)
    s = native.PairSystem()
    A = rs.standard_normal((6, 6)) * 10.0 ** rs.uniform(-8, 8)
    H = A @ A.T
    for i in range(36):
        s.information[i] = H.reshape(-1)[i]
    for i in range(6):
        s.gradient[i] = rs.standard_normal()
    s.cost = float(rs.uniform(0, 1e6))
    s.rows = int(rs.randint(0, 307200))
    return s, H


def test_struct_layout():
    assert C.sizeof(native.PairSystem) == 352
    assert native.PairSystem.rows.offset == 344 and native.PairSystem.flags.offset == 348


def test_numpy_record_matches_the_struct():
    """AlignmentEngine.evaluate_pairs reads the C records through a numpy dtype: same size, same field offsets."""
    from phovo_amd import odometry
    dt = odometry.PAIR_SYSTEM_DTYPE
    assert dt.itemsize == C.sizeof(native.PairSystem)
    for name in ("information", "gradient", "cost", "rows", "flags"):
        assert dt.fields[name][1] == getattr(native.PairSystem, name).offset, name
    s, H = _system(11)
    s.flags = 5
    rec = np.frombuffer(bytes(memoryview(s)), dtype=dt)[0]
    np.testing.assert_array_equal(rec["information"].reshape(6, 6), H)
    assert rec["cost"] == s.cost and rec["rows"] == s.rows and rec["flags"] == 5
    np.testing.assert_array_equal(rec["gradient"], np.array(s.gradient[:]))


@pytest.mark.parametrize("seed", range(5))
def test_format_round_trips(seed):
    s, H = _system(seed)
    ts = 1305031102.175304 + seed * 0.033
    line = native.format_pair_system(ts, s)
    assert "\n" not in line
    f = line.split(" ")
    assert len(f) == 3 + 21
    assert float(f[0]) == ts and int(f[1]) == s.rows and float(f[2]) == s.cost
    iu = np.triu_indices(6)
    np.testing.assert_array_equal(np.array([float(v) for v in f[3:]]), H[iu])


def test_format_special_values():
    s = native.PairSystem()
    s.cost = float("nan")
    s.information[0] = float("inf")
    s.information[1] = -0.0
    line = native.format_pair_system(0.0, s)
    f = line.split(" ")
    assert np.isnan(float(f[2])) and float(f[3]) == np.inf and str(float(f[4])) == "-0.0"


def test_format_capacity_too_small():
    L = native.lib()
    s, _ = _system(7)
    line = native.format_pair_system(1.5, s)
    buf = C.create_string_buffer(len(line) + 1)
    assert L.phovo_pair_system_format(1.5, C.byref(s), buf, len(line) + 1) == native.OK
    assert buf.value.decode() == line
    assert L.phovo_pair_system_format(1.5, C.byref(s), buf, len(line)) == native.E_INVALID_ARGUMENT
    assert L.phovo_pair_system_format(1.5, C.byref(s), buf, 0) == native.E_INVALID_ARGUMENT


def test_null_arguments_are_refused():
    L = native.lib()
    s = native.PairSystem()
    buf = C.create_string_buffer(1024)
    assert L.phovo_pair_system_format(0.0, None, buf, 1024) == native.E_INVALID_ARGUMENT
    assert L.phovo_pair_system_format(0.0, C.byref(s), None, 1024) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_get_pair_system(None, C.byref(s)) == native.E_INVALID_ARGUMENT
    src = (C.c_int * 1)(0)
    st = (C.c_double * 6)()
    assert L.phovo_engine_evaluate_pairs(None, 1, src, src, st, 0, C.byref(s)) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_evaluate_pairs(None, 0, None, None, None, 0, None) == native.E_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def vo_app():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps"),
                           os.path.join(ROOT, "apps", "bin", "PhotoconsistencyVisualOdometry")])
    return os.path.join(ROOT, "apps", "bin", "PhotoconsistencyVisualOdometry")


@pytest.mark.parametrize("extra,needle", [
    (["--batch", "--gpus", "2", "--information", "i.txt"], "--information runs on one device"),
    (["--batch", "--rccl", "--information", "i.txt"], "--information runs on one device"),
    (["--information", "i.txt", "--method", "biobjective"], "--information needs --method analytic"),
])
def test_app_usage_errors(vo_app, tmp_path, extra, needle):
    r = subprocess.run([vo_app, "cfg.yml", str(tmp_path), str(tmp_path / "t.txt")] + extra, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert needle in r.stderr
    assert not (tmp_path / "t.txt").exists()


def test_app_usage_text_names_the_flag(vo_app):
    r = subprocess.run([vo_app], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--information <file>" in r.stdout
