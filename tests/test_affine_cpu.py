"""The affine-illumination checker (tests/affine_ref.py) against itself, against the twin's bilinear-corrected rows it is
built on, against finite differences, and -- qualitatively -- against the ground truth of a pair whose exposure changed.
No GPU."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import se3, synthetic
from oracle import numpy_twin as twin

import affine_ref as ar


def tiny_case(seed, W=9, H=7, spread=1.0):
    """Random planes, depths with gate rejects (too near, too far, NaN) and a motion large enough, for the image size, to
    push pixels out of bounds and into every clamp band."""
    rs = np.random.RandomState(seed)
    K = np.array([[60.0, 0, (W - 1) / 2.0], [0, 55.0, (H - 1) / 2.0], [0, 0, 1]])
    d0 = rs.uniform(0.8, 3.0, (H, W))
    d0.reshape(-1)[rs.choice(W * H, 3, replace=False)] = [0.1, 7.0, np.nan]
    planes = (rs.uniform(0, 1, (H, W)), d0, rs.uniform(0, 1, (H, W)), rs.normal(0, 1, (H, W)), rs.normal(0, 1, (H, W)))
    state = np.concatenate([rs.uniform(-0.02, 0.02, 3) * spread, rs.uniform(-0.03, 0.03, 3) * spread,
                            [rs.uniform(-0.3, 0.3), rs.uniform(-0.1, 0.1)]])
    return planes, K, state


def test_loop_and_vectorised_forms_agree_and_reach_every_branch():
    seen, gate, oob = set(), 0, 0
    for seed in range(12):
        planes, K, state = tiny_case(seed, spread=1.0 + seed % 3)
        r, J, rows = ar.rows_vectorised(planes, 0, K, state)
        rl, Jl, rowsl, bands, stats = ar.rows_loop(planes, 0, K, state)
        np.testing.assert_array_equal(rows, rowsl)
        np.testing.assert_allclose(r, rl, rtol=0, atol=1e-12)
        np.testing.assert_allclose(J, Jl, rtol=0, atol=1e-12 * max(1.0, np.abs(Jl).max()))
        for b in bands.values():
            seen |= b
        gate += stats["gate"]
        oob += stats["oob"]
    assert seen == {"c-", "c+", "r-", "r+"}, seen
    assert gate >= 12 * 3 and oob > 0


def test_pose_block_at_zero_gain_and_offset_is_the_twins_bilinear_corrected_system():
    for seed in range(4):
        planes, K, state = tiny_case(100 + seed)
        state[6:] = 0.0
        r, J, rows = ar.rows_vectorised(planes, 0, K, state)
        res, J6 = twin.normal_equations_bilinear(planes, 0, K, state[:6], corrected=True)
        np.testing.assert_array_equal(r, res)
        np.testing.assert_array_equal(J[:, :6], J6)
        np.testing.assert_array_equal(J[:, :6].T @ J[:, :6], J6.T @ J6)
        np.testing.assert_array_equal(J[:, :6].T @ r, J6.T @ res)
        assert rows.sum() > 8


def test_jacobian_against_central_differences():
    """tests/test_jacobian_kat.py isolates the warp Jacobian with constant gradient planes; the same idea makes finite
    differences of the RESIDUAL meaningful here: on I1 = a c + b r + c0 with GX1 = a, GY1 = b the bilinear sample is the
    ramp itself wherever no tap is clamped, so dr/dpose is exactly GX1 du + GY1 dv.  Step 1e-6: the truncation error of a
    central difference is h^2 |r'''| / 6 ~ 1e-12 x O(10) and its rounding error eps |r| / h ~ 2e-10; the bar is 1e-7 of the
    largest entry of the column (entries are O(1..100)), three orders above both.  The last two columns are exact: the
    residual is linear in alpha and beta."""
    W, H = 12, 9
    rs = np.random.RandomState(3)
    K = np.array([[60.0, 0, 5.5], [0, 55.0, 4.0], [0, 0, 1]])
    cc, rr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    a, b = 0.03, -0.02
    planes = (rs.uniform(0, 1, (H, W)), rs.uniform(1.0, 3.0, (H, W)), a * cc + b * rr + 0.4,
              np.full((H, W), a), np.full((H, W), b))
    state = np.array([0.004, -0.003, 0.005, 0.004, -0.003, 0.002, -0.15, 0.05])
    r, J, rows, bands, _ = ar.rows_loop(planes, 0, K, state)
    inner = np.array([rows[k] and not bands[k] for k in range(W * H)])
    assert inner.sum() > 40
    h = 1e-6
    for j in range(8):
        e = np.zeros(8); e[j] = h
        rp, _, rowsp = ar.rows_vectorised(planes, 0, K, state + e)
        rm, _, rowsm = ar.rows_vectorised(planes, 0, K, state - e)
        np.testing.assert_array_equal(rowsp, rows)
        np.testing.assert_array_equal(rowsm, rows)
        fd = (rp - rm) / (2 * h)
        bar = 1e-7 * max(1.0, np.abs(J[inner, j]).max())
        np.testing.assert_allclose(fd[inner], J[inner, j], rtol=0, atol=bar)
    np.testing.assert_array_equal(J[rows, 6], -planes[0].reshape(-1)[rows])
    np.testing.assert_array_equal(J[rows, 7], -1.0)


GAIN, OFFSET = 0.8, 20.0 / 255.0            # keeps any u8 input in range: 0.8 x 255 + 20 = 224


def exposure_pair(seed=31, w=160, h=120):
    p = synthetic.make_pair(seed, w, h, holes=0.02)
    p["gray1"] = np.rint(GAIN * p["gray1"].astype(np.float64) + OFFSET * 255.0).astype(np.uint8)
    return p


def test_gain_and_offset_are_recovered_and_the_pose_improves():
    p = exposure_pair()
    nl = 3
    cfg = dict(num_levels=nl, lam=[1.0] * nl, max_iter=[10] * nl, min_grad=[0.0] * nl)
    pyr = twin.build_pyramids(p["gray0"], p["depth0"], p["gray1"], nl, [0.0625] * nl)
    res = ar.optimize(pyr, p["K"], cfg)
    plain, _, _ = twin.optimize(pyr, p["K"], dict(cfg, bilinear=True, corrected=True))
    err_affine = se3.state_distance(res["state"][:6], p["motion"])
    err_plain = se3.state_distance(plain, p["motion"])
    ab = res["state"][6:]
    print(f"pose error: affine {err_affine:.3e}, bilinear-corrected photometric {err_plain:.3e}; "
          f"(alpha, beta) = ({ab[0]:.4f}, {ab[1]:.4f}), exposure change ({GAIN - 1:.4f}, {OFFSET:.4f})")
    assert res["flags"] == 0
    assert err_affine < err_plain
    assert np.linalg.norm(ab - [GAIN - 1.0, OFFSET]) < np.linalg.norm(ab)
