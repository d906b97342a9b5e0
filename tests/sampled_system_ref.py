"""CPU checker of phovo_engine_evaluate_sampled_pairs, in numpy: H = J^T W J, g = J^T W r, cost = r^T W r and
the row count of the rows the sampled aligners define -- the bilinear extension's (oracle/numpy_twin.py,
normal_equations_bilinear: six columns, either Jacobian, optional Huber weights) and the affine-illumination objective's
(tests/affine_ref.py, rows_vectorised: eight columns).  Test infrastructure, not collected."""
import numpy as np

from oracle import numpy_twin as twin

import affine_ref


def check_against(sys_h, sys_g, rows, cost, ref_h, ref_g, ref_rows, ref_cost):
    """The bars of tests/test_gpu_pair_system.py's _check_against, diag over dim entries.  Returns the ratios to the bars."""
    assert rows == ref_rows, (rows, ref_rows)
    scale = np.max(np.abs(ref_h))
    dh = np.max(np.abs(sys_h - ref_h))
    assert dh <= 1e-10 * scale, (dh, scale)
    bar = 1e-9 * np.sqrt(np.maximum(np.diag(ref_h) * ref_cost, 0.0))
    assert np.all(np.abs(sys_g - ref_g) <= bar), (sys_g - ref_g, bar)
    assert abs(cost - ref_cost) <= 1e-12 * abs(ref_cost), (cost, ref_cost)
    with np.errstate(all="ignore"):
        return dh / scale, float(np.max(np.where(bar > 0, np.abs(sys_g - ref_g) / bar, 0.0)))


def row_mask(planes, level, K, pose, min_depth=0.3, max_depth=5.0):
    """Which source pixels are rows: the twin's own gate and bounds test, read off a run on I0 = 0, I1 = 1 (affine_ref)."""
    i0, d0 = planes[0], planes[1]
    z, o = np.zeros_like(i0), np.ones_like(i0)
    probe, _ = twin.normal_equations_bilinear((z, d0, o, z, z), level, K, np.asarray(pose, dtype=np.float64), min_depth,
                                              max_depth, corrected=True)
    return probe != 0.0


def system6(planes, level, K, state, corrected, delta=None, min_depth=0.3, max_depth=5.0):
    """(H[6,6], g[6], cost, rows) of the bilinear rows at `state`; delta > 0: Huber weights 1 or delta / |r|."""
    state = np.asarray(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        r, J = twin.normal_equations_bilinear(planes, level, K, state, min_depth, max_depth, corrected=corrected)
        rows = row_mask(planes, level, K, state, min_depth, max_depth)
        r, J = r[rows], J[rows]
        w = np.ones_like(r)
        if delta is not None and delta > 0:
            ar = np.abs(r)
            w = np.where(ar <= delta, 1.0, delta / np.where(ar > 0, ar, 1.0))
        Jw = J * w[:, None]
        return Jw.T @ J, Jw.T @ r, float(np.sum(w * r * r)), int(rows.sum())


def system8(planes, level, K, state8, min_depth=0.3, max_depth=5.0):
    """(H[8,8], g[8], cost, rows) of the affine-illumination rows at (pose, alpha, beta)."""
    with np.errstate(all="ignore"):
        r, J, rows = affine_ref.rows_vectorised(planes, level, K, np.asarray(state8, dtype=np.float64), min_depth, max_depth)
        r, J = r[rows], J[rows]
        return J.T @ J, J.T @ r, float(np.sum(r * r)), int(rows.sum())
