"""The inverse-compositional checker (tests/inverse_ref.py) against itself, against central differences and against an
exact matrix exponential; phovo_state_from_pose against phovo_eigen_pose through the library; the new symbol, constant, class
and app method; and the accuracy the formulation was chosen for.  No GPU."""
import ctypes as C
import os
import subprocess

import mpmath
import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, synthetic
from oracle import numpy_twin as twin

import inverse_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_case(seed, W, H):
    """Random planes with gate rejects (too near, too far, NaN) and a motion large enough, for the image size, to push
    pixels out of bounds and into the clamp bands."""
    rs = np.random.RandomState(seed)
    K = np.array([[60.0, 0, (W - 1) / 2.0], [0, 55.0, (H - 1) / 2.0], [0, 0, 1]])
    d0 = rs.uniform(1.5, 2.0, (H, W))
    d0.reshape(-1)[rs.choice(W * H, 3, replace=False)] = [0.1, 7.0, np.nan]
    planes = (rs.uniform(0, 1, (H, W)), d0, rs.normal(0, 1, (H, W)), rs.normal(0, 1, (H, W)), rs.uniform(0, 1, (H, W)))
    state = np.concatenate([rs.uniform(-0.04, 0.04, 3), rs.uniform(-0.05, 0.05, 3)])
    return planes, K, state


@pytest.mark.parametrize("w,h", [(7, 5), (20, 15)])
def test_loop_and_vectorised_forms_agree(w, h):
    rows_total, out_total = 0, 0
    for seed in range(6):
        planes, K, state = tiny_case(seed, w, h)
        R, t = ir.eigen_rt(state)
        rv, Jv, mv = ir.rows_vectorised(planes, 0, K, R, t)
        rl, Jl, ml = ir.rows_loop(planes, 0, K, R, t)
        np.testing.assert_array_equal(mv, ml)
        np.testing.assert_allclose(rv, rl, rtol=0, atol=1e-13)
        np.testing.assert_allclose(Jv, Jl, rtol=0, atol=1e-12 * max(1.0, np.abs(Jl).max()))
        assert not Jv[~mv].any() and not rv[~mv].any()
        rows_total += int(mv.sum())
        out_total += int((~mv).sum())
    assert rows_total > 0 and out_total > 3 * 6          # more than the gate rejects: some pixels leave the image


def test_row_is_the_derivative_of_the_source_image_under_a_twist():
    """J_k = d/d(delta) I0(pi(Exp(delta) p_k)) at delta = 0 for a smooth analytic I0, against central differences with
    h = 1e-5.  Bar: the difference quotient's truncation h^2 / 6 |f'''| plus its rounding eps |f| / h.  Along a twist
    direction the pixel position moves by at most |d(u, v)/d(delta)| <= 60 * 2.5 = 150 pixels per unit (fx / pz times
    (1 + |p|^2 / pz^2) on this 9x7 frame), the image has spatial frequency <= 0.13 rad per pixel, so |f'''| <= (0.13 * 150)^3
    ~ 7.5e3 and the truncation is below 1.3e-7; the rounding is 1e-11.  2e-7 absolute, on rows of size ~10."""
    W, H = 9, 7
    K = np.array([[60.0, 0, 4.2], [0, 55.0, 2.9], [0, 0, 1]])
    fx, fy, ox, oy = 60.0, 55.0, 4.2, 2.9

    def img(u, v):
        return 0.5 + 0.3 * np.sin(0.11 * u + 0.07 * v) + 0.2 * np.cos(0.05 * u - 0.09 * v)

    def grad(u, v):
        return (0.3 * 0.11 * np.cos(0.11 * u + 0.07 * v) - 0.2 * 0.05 * np.sin(0.05 * u - 0.09 * v),
                0.3 * 0.07 * np.cos(0.11 * u + 0.07 * v) + 0.2 * 0.09 * np.sin(0.05 * u - 0.09 * v))
    rs = np.random.RandomState(3)
    cc, rr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d0 = rs.uniform(1.2, 2.5, (H, W))
    gx0, gy0 = grad(cc, rr)
    planes = (img(cc, rr), d0, gx0, gy0, img(cc, rr))
    _, J, rows = ir.rows_vectorised(planes, 0, K, np.eye(3), np.zeros(3))
    assert rows.all()
    h = 1e-5
    worst = 0.0
    for k in range(W * H):
        r_, c_ = divmod(k, W)
        pz = d0[r_, c_]
        p = np.array([(c_ - ox) * pz / fx, (r_ - oy) * pz / fy, pz])

        def at(delta):
            ER, Et = ir.se3_exp(delta)
            P = ER @ p + Et
            return img(fx * P[0] / P[2] + ox, fy * P[1] / P[2] + oy)
        for j in range(6):
            e = np.zeros(6)
            e[j] = h
            worst = max(worst, abs((at(e) - at(-e)) / (2 * h) - J[k, j]))
    print(f"largest |central difference - J| = {worst:.3e}, largest |J| = {np.abs(J).max():.3e}")
    assert worst <= 2e-7


def _expm_exact(xi):
    mpmath.mp.dps = 60
    nu, w = [mpmath.mpf(float(v)) for v in xi[:3]], [mpmath.mpf(float(v)) for v in xi[3:]]
    M = mpmath.matrix([[0, -w[2], w[1], nu[0]], [w[2], 0, -w[0], nu[1]], [-w[1], w[0], 0, nu[2]], [0, 0, 0, 0]])
    E = mpmath.expm(M, method="taylor")
    return np.array([[float(E[i, j]) for j in range(4)] for i in range(3)])


@pytest.mark.parametrize("theta", [0.0, 1e-9, 1e-5, 9.9e-5, 1.01e-4, 0.3, 3.0])
def test_se3_exp_against_the_exact_matrix_exponential(theta):
    """Both sides of the Taylor switch (|omega|^2 = 1e-8 at |omega| = 1e-4).  Bar: 4 ulp of the largest entry."""
    assert (theta * theta < ir.TAYLOR_BELOW) == (theta < 1e-4)
    worst = 0.0
    for seed in range(8):
        rs = np.random.RandomState(seed)
        axis = rs.normal(size=3)
        axis /= np.linalg.norm(axis)
        xi = np.concatenate([rs.uniform(-0.5, 0.5, 3), theta * axis])
        ER, Et = ir.se3_exp(xi)
        got = np.concatenate([ER, Et.reshape(3, 1)], axis=1)
        exact = _expm_exact(xi)
        bar = 4 * np.spacing(np.abs(exact).max())
        err = np.abs(got - exact).max()
        worst = max(worst, err / bar)
        assert err <= bar, (seed, err, bar)
    print(f"theta {theta}: worst error / bar = {worst:.3f}")


def _through_the_library(state):
    L = native.lib()
    dp = C.POINTER(C.c_double)
    rt, back = np.zeros(16), np.zeros(6)
    s = np.ascontiguousarray(state, dtype=np.float64)
    assert L.phovo_eigen_pose(s.ctypes.data_as(dp), rt.ctypes.data_as(dp)) == 0
    assert L.phovo_state_from_pose(rt.ctypes.data_as(dp), back.ctypes.data_as(dp)) == 0
    return rt.reshape(4, 4), back


def test_state_from_pose_inverts_eigen_pose():
    rs = np.random.RandomState(11)
    worst = 0.0
    for _ in range(200):
        s = np.concatenate([rs.uniform(-2, 2, 3), rs.uniform(-np.pi, np.pi, 1), rs.uniform(-1.5, 1.5, 1),
                            rs.uniform(-np.pi, np.pi, 1)])
        rt, back = _through_the_library(s)
        worst = max(worst, np.abs(back - s).max())
        np.testing.assert_allclose(native.state_from_pose(rt), back, rtol=0, atol=0)
        np.testing.assert_allclose(ir.state_from_pose(rt[:3, :3], rt[:3, 3]), back, rtol=0, atol=1e-15)
    print(f"largest |state_from_pose(eigen_pose(s)) - s| = {worst:.3e}")
    assert worst <= 1e-14
    # yaw and roll at +-pi: the angle comes back as +-pi (the same rotation), not as something near 0
    for yaw in (np.pi, -np.pi):
        for roll in (np.pi, -np.pi):
            s = np.array([0.1, -0.2, 0.3, yaw, 0.25, roll])
            rt, back = _through_the_library(s)
            assert np.abs(np.abs(back[[3, 5]]) - np.pi).max() <= 1e-14
            assert np.abs(back[[0, 1, 2, 4]] - s[[0, 1, 2, 4]]).max() <= 1e-14
            rt2, _ = _through_the_library(back)
            assert np.abs(rt2 - rt).max() <= 1e-15
    L = native.lib()
    assert L.phovo_state_from_pose(None, None) == native.E_INVALID_ARGUMENT
    z = np.zeros(16)
    assert L.phovo_state_from_pose(z.ctypes.data_as(C.POINTER(C.c_double)), None) == native.E_INVALID_ARGUMENT


def test_the_surface_is_there():
    assert native.OBJECTIVE_INVERSE_COMPOSITIONAL == 5
    assert native.LAUNCH_KINDS[10] == "inverse"
    assert hasattr(native.lib(), "phovo_state_from_pose")
    assert issubclass(odometry.CPhotoconsistencyOdometryInverse, odometry.CPhotoconsistencyOdometryAnalytic)
    header = open(os.path.join(ROOT, "include", "phovo_hip.h")).read()
    assert "#define PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL 5" in header
    assert "PHOVO_LAUNCH_INVERSE = 10" in header
    assert "int phovo_state_from_pose(const double rt[16], double state[6]);" in header
    for d in ("phovo", "shim"):
        assert os.path.exists(os.path.join(ROOT, "include", d, "CPhotoconsistencyOdometryInverse.h"))


@pytest.fixture(scope="module")
def apps():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])
    return os.path.join(ROOT, "apps", "bin")


def test_the_apps_name_the_method(apps):
    for app in ("PhotoconsistencyVisualOdometry", "PhotoconsistencyFrameAlignment"):
        r = subprocess.run([os.path.join(apps, app)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "|inverse|" in r.stdout


@pytest.mark.parametrize("flag,needle", [
    ("--information", "--information needs --method analytic"),
    ("--system", "--system needs bilinear sampling or --method affine"),
    ("--geometric-system", "--geometric-system needs --method geometric"),
    ("--objective-system", "--objective-system needs --method ceres or --method biobjective"),
])
def test_the_system_flags_refuse_the_method(apps, tmp_path, flag, needle):
    r = subprocess.run([os.path.join(apps, "PhotoconsistencyVisualOdometry"), "cfg.yml", str(tmp_path), str(tmp_path / "t.txt"),
                        "--method", "inverse", flag, "s.txt"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert needle in r.stderr
    assert not (tmp_path / "t.txt").exists()


def twin_pyramid(p, nl, scale=0.0625):
    """(the twin's pyramid, the checker's): the source's gradient planes are the Scharr of its own intensity level."""
    pyr = twin.build_pyramids(p["gray0"], p["depth0"], p["gray1"], nl, [scale] * nl)
    return pyr, [(i0, d0) + tuple(twin.scharr(i0, scale)) + (i1,) for i0, d0, i1, _, _ in pyr]


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_accuracy_against_the_generators_motion(seed):
    """160x120, 3 levels x 10 iterations, lambda 1: the checker's largest pose error against the motion the pair was
    rendered with is at most 1e-3 and below that of the reference's nearest / scatter aligner (the numpy twin)."""
    nl = 3
    cfg = dict(num_levels=nl, lam=[1.0] * nl, max_iter=[10] * nl, min_grad=[0.0] * nl, min_depth=0.3, max_depth=5.0)
    p = synthetic.make_pair(seed, 160, 120)
    pyr, ipyr = twin_pyramid(p, nl)
    ref = ir.optimize(ipyr, p["K"], cfg)
    scatter, _, _ = twin.optimize(pyr, p["K"], cfg)
    err, err_scatter = np.abs(ref["state"] - p["motion"]).max(), np.abs(scatter - p["motion"]).max()
    print(f"seed {seed}: inverse-compositional {err:.3e}, nearest / scatter {err_scatter:.3e}, cond {ref['cond']:.3e}")
    assert ref["flags"] == 0 and ref["iterations"] == [10] * nl
    assert err <= 1e-3
    assert err < err_scatter
