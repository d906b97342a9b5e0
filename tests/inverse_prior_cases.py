"""Fixtures of the Gaussian pose prior of the inverse-compositional objectives (phovo_engine_enqueue_align_prior, DESIGN.md
§24), shared by tests/test_inverse_prior_cpu.py (which holds every one of them to the properties the GPU file relies on:
cond(H'), the distance to the gradient thresholds, the angle keep-outs, the robust counts' margins -- on CPU pyramids) and
tests/test_gpu_inverse_prior.py (which runs them on the device).  TEST INFRASTRUCTURE ONLY, not collected."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic

import inverse_edges as ie
import inverse_ref as ir

MARGIN_FLOOR = ie.MARGIN_FLOOR            # no iteration comes this close (relative) to its gradient threshold
MAX_PRIOR_ANGLE = 3.0                     # the accuracy contract of Log: |omega| of every e formed stays below
SKEW_AXIS = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])      # no coordinate axis, no plane of two
PRIOR_STATE = np.array([0.012, -0.007, 0.009, 0.005, -0.004, 0.006])             # a prior pose away from zero and from the truth


def lambda_iso(weight):
    return weight * np.eye(6)


def lambda_full(seed, weight):
    """A full, non-diagonal, symmetric positive definite matrix: weight * (M M^T / 6 + I / 2), M from U(-1, 1)."""
    m = np.random.RandomState(seed).uniform(-1.0, 1.0, (6, 6))
    return weight * (m @ m.T / 6.0 + 0.5 * np.eye(6))


def with_fy(K, factor):
    """K with fy = factor * fx's row scaled: the row's J[0] = gx fx / pz and J[1] = gy fy / pz then differ."""
    K = np.array(K, dtype=np.float64)
    K[1, 1] *= factor
    return K


def small_pair(seed, w, h):
    return synthetic.make_pair(seed, w, h, holes=0.02, trans=0.01, rot=0.005)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
# name -> (pair, fy / fx, levels, max_iter, min_grad, lambda_optimization_step, level_scale, Lambda).  Lambda's weight is a
# fraction of H's translation diagonal on the finest level (H grows with the row count), so that data and prior both move
# the pose; among the cases are fy != fx, lambda != 1 and level scales that are not all 1.  The thresholds of the two-level
# case end both levels (1 < iterations < max) under BOTH objectives: test_inverse_prior_cpu.py asserts that.
PARITY = {
    "8x8 iso": (lambda: small_pair(1, 8, 8), 1.0, 1, [5], [0.0], [1.0], [1.0], lambda_iso(5.0)),
    "7x5 full": (lambda: small_pair(1, 7, 5), 1.1, 1, [5], [0.0], [0.8], [0.5], lambda_full(11, 2.0)),
    "24x20 full": (lambda: small_pair(1, 24, 20), 1.0, 1, [5], [0.0], [0.9], [2.0], lambda_full(12, 300.0)),
    "24x20 two levels by threshold": (lambda: small_pair(1, 24, 20), 1.1, 2, [12, 12], [0.6, 0.1], [0.9, 0.8], [1.0, 0.5],
                                      lambda_iso(200.0)),
    "75x53 full": (lambda: small_pair(1, 75, 53), 1.1, 1, [5], [0.0], [0.9], [0.7], lambda_full(13, 3000.0)),
    "80x60 iso": (lambda: small_pair(1, 80, 60), 1.0, 1, [5], [0.0], [1.0], [1.5], lambda_iso(4000.0)),
    # (seed 1 comes within 2e-8 bins of a bin's edge under objective 6; seed 2 is the first that keeps the floors)
    "160x120 three levels": (lambda: synthetic.make_pair(2, 160, 120, holes=0.02), 1.1, 3, [6, 6, 6], [0.0] * 3,
                             [1.0, 0.9, 0.8], [1.0, 0.5, 2.0], lambda_full(14, 10000.0)),
}


def parity_problem(name):
    make, fy, nl, mi, mg, lam, scales, Lam = PARITY[name]
    p = make()
    return dict(p=p, K=with_fy(p["K"], fy), nl=nl, mi=mi, mg=mg, lam=lam, scales=scales, Lambda=Lam, prior=PRIOR_STATE)


def cfg(mi, mg=None, lam=None):
    return ie.cfg(mi, mg, lam=lam)


# ---- 3. Log's regimes: a constant source, lambda = 1, one iteration lands on the prior ----------------------------------
LOG_W, LOG_H, LOG_SEED = 24, 20, 41
LOG_ANGLES = ie.EXP_TARGETS               # 5e-5 ... 3.0 rad about SKEW_AXIS: both sides of the series switch, every sin / cos branch
LOG_TRANSLATION = np.array([0.04, -0.03, 0.05])
LOG_INIT = np.array([0.02, 0.01, -0.015, -0.03, 0.06, 0.02])      # the start: not the identity, so that a left-hand error differs


def log_prior_state(angle):
    """The state of T_init Exp((LOG_TRANSLATION, angle * SKEW_AXIS)): a relative rotation of `angle` from the start LOG_INIT."""
    R, t = ir.eigen_rt(LOG_INIT)
    ER, Et = ir.se3_exp(np.concatenate([LOG_TRANSLATION, angle * SKEW_AXIS]))
    return ir.state_from_pose(R @ ER, R @ Et + t)


def constant_source_pair(seed=LOG_SEED, w=LOG_W, h=LOG_H):
    """A pair whose source intensity is constant: zero gradient planes, H and g exactly zero, every depth valid."""
    p = synthetic.make_pair(seed, w, h)
    p["gray0"] = np.full_like(p["gray0"], 128)
    return p


# ---- 4. five, six and seven rows (inverse_edges.rows_problem) under a prior ---------------------------------------------
ROWS_LAMBDA = lambda_full(15, 0.05)       # H of these systems has a diagonal of 1e-2 ... 1
ROWS_CASES = [(layout, count, const) for layout in ie.ROWS_LAYOUTS for count, const in ((5, False), (6, False), (7, False),
                                                                                         (5, True), (6, True))]

# ---- 5. the work queue: inverse_edges' four pairs (D: all-NaN source depth), a prior per POSITION -----------------------
WQ_LAMBDAS = 5                            # distinct information matrices of the list; index 0 is Lambda = 0
WQ_PRIORS = 6                             # distinct prior poses
WQ_MAX_ITER, WQ_MIN_GRAD = ie.WQ_MAX_ITER, ie.WQ_MIN_GRAD


def work_queue_priors(n, seed=3):
    """(prior_states[WQ_PRIORS, 6], lambdas[WQ_LAMBDAS, 6, 6], pick_state[n], pick_lambda[n])."""
    rs = np.random.RandomState(seed)
    states = rs.uniform(-1.0, 1.0, (WQ_PRIORS, 6)) * np.array([0.01, 0.01, 0.01, 0.005, 0.005, 0.005])
    lambdas = np.stack([np.zeros((6, 6)), lambda_iso(100.0), lambda_full(21, 150.0), lambda_full(22, 40.0), lambda_iso(1e4)])
    return states, lambdas, rs.randint(0, WQ_PRIORS, n), rs.randint(0, WQ_LAMBDAS, n)
