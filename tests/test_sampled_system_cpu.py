"""CPU tests of the sampled-system surface (no GPU needed): the numpy checker tests/sampled_system_ref.py against the C
oracle's one-iteration traces, the record layout, phovo_sampled_system_format, the NULL-argument refusals and the
VisualOdometry app's usage errors for --system."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, synthetic
from oracle import oracle

import affine_edges
import sampled_system_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(32, 24), (32, 32), (41, 25), (75, 53), (160, 120)]


@pytest.fixture(scope="module")
def problems():
    out = {}
    for w, h in SIZES:
        p = synthetic.make_pair(33, w, h, holes=0.02)
        out[(w, h)] = (p, affine_edges.oracle_pyramid(p, 1)[0])
    return out


def _trace_system(planes, K, state, corrected, delta, min_depth=0.3, max_depth=5.0):
    """rows, H, g of ONE oracle iteration of the bilinear extension from `state`."""
    cfg = oracle.make_config(num_levels=1, max_iter=[1], min_grad=[0.0], min_depth=min_depth, max_depth=max_depth)
    _, _, tr = oracle.optimize(cfg, K, *[[a] for a in planes], init_state=state, want_trace=True,
                               huber_delta=None if delta is None else [delta], bilinear=True, corrected=corrected)
    assert len(tr) == 1
    return tr[0]["valid_pixels"], tr[0]["hessian"], tr[0]["gradient"]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("corrected", [False, True])
@pytest.mark.parametrize("delta", [None, 0.03])
def test_checker_matches_the_oracle_trace(problems, w, h, corrected, delta):
    p, planes = problems[(w, h)]
    for state in (np.zeros(6), p["motion"]):
        rows, H, g = _trace_system(planes, p["K"], state, corrected, delta)
        Hc, gc, cost, rows_c = ref.system6(planes, 0, p["K"], state, corrected, delta)
        assert rows > 6 and cost > 0
        # (the checker's own cost stands in for the oracle's, which its trace does not carry)
        print(w, h, corrected, delta, ref.check_against(Hc, gc, rows_c, cost, H, g, rows, cost))


def test_the_two_jacobians_differ_by_far_more_than_the_bar(problems):
    """At a non-zero translation the slip changes H by more than 1e6 H-bars: a device that ignored jacobian_corrected
    cannot pass either way."""
    p, planes = problems[(160, 120)]
    Hs, _, _, _ = ref.system6(planes, 0, p["K"], p["motion"], False)
    Hc, _, _, _ = ref.system6(planes, 0, p["K"], p["motion"], True)
    bar = 1e-10 * min(np.max(np.abs(Hs)), np.max(np.abs(Hc)))
    assert np.max(np.abs(Hs - Hc)) > 1e6 * bar
    H0s, _, _, _ = ref.system6(planes, 0, p["K"], np.zeros(6), False)      # (at x = 0 the slip vanishes)
    H0c, _, _, _ = ref.system6(planes, 0, p["K"], np.zeros(6), True)
    np.testing.assert_array_equal(H0s, H0c)


@pytest.mark.parametrize("w,h", [(41, 25), (75, 53)])
def test_eight_columns_extend_the_corrected_six(problems, w, h):
    p, planes = problems[(w, h)]
    H6, g6, cost6, rows6 = ref.system6(planes, 0, p["K"], p["motion"], True)
    H8, g8, cost8, rows8 = ref.system8(planes, 0, p["K"], np.concatenate([p["motion"], [0.0, 0.0]]))
    ref.check_against(H8[:6, :6], g8[:6], rows8, cost8, H6, g6, rows6, cost6)      # (two matrix products: not bit for bit)
    assert H8[7, 7] == rows8
    i0 = planes[0].reshape(-1)[ref.row_mask(planes, 0, p["K"], p["motion"])]
    assert abs(H8[6, 7] - i0.sum()) <= 1e-12 * i0.sum() and abs(H8[6, 6] - (i0 * i0).sum()) <= 1e-12 * (i0 * i0).sum()
    # H does not depend on alpha, beta; the residual does
    H8b, g8b, cost8b, _ = ref.system8(planes, 0, p["K"], np.concatenate([p["motion"], [-0.2, 0.08]]))
    np.testing.assert_array_equal(H8b, H8)
    assert cost8b != cost8


# ---- the record ----------------------------------------------------------------------------------------------------
def _system(seed, dim):
    rs = np.random.RandomState(seed)
    s = native.SampledSystem()
    A = rs.standard_normal((dim, dim)) * 10.0 ** rs.uniform(-8, 8)
    H = np.zeros((8, 8))
    H[:dim, :dim] = A @ A.T
    for i in range(64):
        s.information[i] = H.reshape(-1)[i]
    for i in range(dim):
        s.gradient[i] = rs.standard_normal()
    s.cost = float(rs.uniform(0, 1e6))
    s.rows = int(rs.randint(0, 307200))
    s.dim = dim
    return s, H


def test_struct_layout():
    S = native.SampledSystem
    assert native.SYSTEM_MAX_DIM == 8
    assert C.sizeof(S) == 600
    assert [getattr(S, f).offset for f in ("information", "gradient", "cost", "rows", "flags", "dim", "reserved")] == \
        [0, 512, 576, 584, 588, 592, 596]


def test_numpy_record_matches_the_struct():
    from phovo_amd import odometry
    dt = odometry.SAMPLED_SYSTEM_DTYPE
    assert dt.itemsize == C.sizeof(native.SampledSystem)
    for name in ("information", "gradient", "cost", "rows", "flags", "dim", "reserved"):
        assert dt.fields[name][1] == getattr(native.SampledSystem, name).offset, name
    s, H = _system(11, 8)
    s.flags = 5
    rec = np.frombuffer(bytes(memoryview(s)), dtype=dt)[0]
    np.testing.assert_array_equal(rec["information"].reshape(8, 8), H)
    assert rec["cost"] == s.cost and rec["rows"] == s.rows and rec["flags"] == 5 and rec["dim"] == 8
    np.testing.assert_array_equal(rec["gradient"], np.array(s.gradient[:]))


def test_format_exact_text():
    for dim in (6, 8):
        s = native.SampledSystem()
        s.dim, s.rows, s.cost = dim, 1234, 0.1
        for a in range(8):
            for b in range(8):
                s.information[8 * a + b] = (10 * min(a, b) + max(a, b)) / 4.0 if max(a, b) < dim else 0.0
        want = ["1305031102.1753039", "1234", "0.10000000000000001", str(dim)]
        want += ["%.17g" % ((10 * a + b) / 4.0) for a in range(dim) for b in range(a, dim)]
        assert native.format_sampled_system(1305031102.175304, s) == " ".join(want)
        assert len(want) == 4 + dim * (dim + 1) // 2


@pytest.mark.parametrize("seed,dim", [(0, 6), (1, 8), (2, 6), (3, 8)])
def test_format_round_trips(seed, dim):
    s, H = _system(seed, dim)
    ts = 1305031102.175304 + seed * 0.033
    line = native.format_sampled_system(ts, s)
    assert "\n" not in line
    f = line.split(" ")
    assert len(f) == 4 + dim * (dim + 1) // 2
    assert float(f[0]) == ts and int(f[1]) == s.rows and float(f[2]) == s.cost and int(f[3]) == dim
    np.testing.assert_array_equal(np.array([float(v) for v in f[4:]]), H[:dim, :dim][np.triu_indices(dim)])


def test_format_capacity():
    L = native.lib()
    s, _ = _system(7, 8)
    line = native.format_sampled_system(1.5, s)
    buf = C.create_string_buffer(len(line) + 1)
    assert L.phovo_sampled_system_format(1.5, C.byref(s), buf, len(line) + 1) == native.OK
    assert buf.value.decode() == line
    assert L.phovo_sampled_system_format(1.5, C.byref(s), buf, len(line)) == native.E_INVALID_ARGUMENT
    assert L.phovo_sampled_system_format(1.5, C.byref(s), buf, 0) == native.E_INVALID_ARGUMENT
    # the capacity the header states always suffices: the longest doubles there are, in every slot
    for i in range(64):
        s.information[i] = -1.7976931348623157e308
    s.cost, s.rows = -2.2250738585072014e-308, -2147483648
    big = C.create_string_buffer(1024)
    assert L.phovo_sampled_system_format(-1.7976931348623157e308, C.byref(s), big, 1024) == native.OK


def test_null_and_bad_arguments_are_refused():
    L = native.lib()
    s = native.SampledSystem()
    s.dim = 6
    buf = C.create_string_buffer(1024)
    assert L.phovo_sampled_system_format(0.0, None, buf, 1024) == native.E_INVALID_ARGUMENT
    assert L.phovo_sampled_system_format(0.0, C.byref(s), None, 1024) == native.E_INVALID_ARGUMENT
    s.dim = 7
    assert L.phovo_sampled_system_format(0.0, C.byref(s), buf, 1024) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_get_sampled_system(None, C.byref(s)) == native.E_INVALID_ARGUMENT
    src = (C.c_int * 1)(0)
    st = (C.c_double * 8)()
    assert L.phovo_engine_evaluate_sampled_pairs(None, 1, src, src, st, 6, 0, C.byref(s)) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_evaluate_sampled_pairs(None, 0, None, None, None, 8, 0, None) == native.E_INVALID_ARGUMENT
    assert b"null engine" in L.phovo_last_error()


# ---- the app ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vo_app():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps"),
                           os.path.join(ROOT, "apps", "bin", "PhotoconsistencyVisualOdometry")])
    return os.path.join(ROOT, "apps", "bin", "PhotoconsistencyVisualOdometry")


CFG4 = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")
CERES = os.path.join(ROOT, "tests", "golden", "ceres", "config_3_level_optimization_ceres.yml")


@pytest.mark.parametrize("cfg,extra,needle", [
    (CFG4, ["--batch", "--gpus", "2", "--system", "s.txt", "--method", "affine"], "--system runs on one device"),
    (CFG4, ["--batch", "--rccl", "--system", "s.txt", "--method", "affine"], "--system runs on one device"),
    (CFG4, ["--system", "s.txt", "--method", "biobjective"], "--system needs bilinear sampling or --method affine"),
    (CERES, ["--system", "s.txt", "--method", "ceres"], "--system needs bilinear sampling or --method affine"),
    (CFG4, ["--system", "s.txt"], "--system needs bilinear sampling or --method affine"),     # nearest / scatter yml
    (CFG4, ["--system", "s.txt", "--method", "analytic", "--batch"], "--system needs bilinear sampling or --method affine"),
    (CFG4, ["--information", "i.txt", "--method", "affine"], "--information needs --method analytic"),     # (unchanged)
])
def test_app_usage_errors(vo_app, tmp_path, cfg, extra, needle):
    r = subprocess.run([vo_app, cfg, str(tmp_path), str(tmp_path / "t.txt")] + extra, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert needle in r.stderr
    assert not (tmp_path / "t.txt").exists()


def test_app_usage_text_names_the_flag(vo_app):
    r = subprocess.run([vo_app], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--system <file>" in r.stdout and "--information <file>" in r.stdout
