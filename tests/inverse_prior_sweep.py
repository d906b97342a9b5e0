"""Randomised draws of the Gaussian pose prior of the inverse-compositional objectives (gn_inverse_prior_kernel.hip,
phovo_engine_enqueue_align_prior) for tests/test_gpu_inverse_prior_sweep.py, with the checker's verdict on
which pairs a device comparison may rely on.  tests/test_inverse_prior_sweep_cpu.py holds the draw to its cap and to the
classes it must contain, on CPU pyramids.  TEST INFRASTRUCTURE ONLY, not collected.

A case: one image pair (7..48 x 5..40, one level below 16 pixels on a side, else 1..3; holes 0..5 %; fy / fx 1.0 or 1.1), 1, 3
or 12 pairs per enqueue over its two frames, each with a start of its own (up to 0.01 m, 0.005 rad), a prior pose of its own
(up to 0.02 m; angles up to 0.01 rad or, one in three, up to 0.3 rad) and an information matrix of its own -- zero, isotropic,
full, rotation-only, translation-only, or a diagonal spanning 1e-3 .. 1e3 around its weight; the weight is 10^U(-2, 1) times
the checker's H[0, 0] on the finest level at the identity.  Per level a scale from {0, 0.5, 1, 2}, a step length from
[0.5, 1] and 2..6 iterations; one case in three has thresholds at 0.3 of the checker's first-iteration ||g'|| on the level
(pair 0, objective 5).  Zero and semidefinite matrices are drawn only from 24x20 up: the data alone carries the directions
the prior leaves free."""
import functools

import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic

import inverse_edges as ie
import inverse_prior_cases as cases
import inverse_prior_ref as pr
import inverse_ref as ir
import inverse_robust_cases as rcases

SEED = 2027                               # the first of 2024 .. 2027 whose draw sets no pair aside on CPU pyramids
N_CASES = 150
CHUNK = 25
CHUNKS = N_CASES // CHUNK
SET_ASIDE_CAP = 0.05
COND_CAP = 1e8
LAMBDA_CLASSES = ("zero", "iso", "full", "rotation_only", "translation_only", "diagonal")
DEFINITE_CLASSES = ("iso", "full", "diagonal")                   # what a size under 24x20 draws from
LEVEL_SCALES = (0.0, 0.5, 1.0, 2.0)
PAIR_COUNTS = (1, 3, 12)
WIDE_ANGLE = 0.3


def draw(i):
    """The raw draw of case i: everything that needs no image."""
    rs = np.random.RandomState((SEED * 100003 + i) % (2 ** 32))
    w, h = int(rs.randint(7, 49)), int(rs.randint(5, 41))
    nl = 1 if min(w, h) < 16 else int(rs.randint(1, 4))
    holes, fy = float(rs.uniform(0.0, 0.05)), float(rs.choice([1.0, 1.1]))
    n = int(rs.choice(PAIR_COUNTS))
    inits = rs.uniform(-1.0, 1.0, (n, 6)) * np.array([0.01] * 3 + [0.005] * 3)
    inits[np.abs(inits) < 1e-5] = 1e-5                          # non-zero
    wide = rs.randint(0, 3, n) == 0
    priors = rs.uniform(-1.0, 1.0, (n, 6)) * np.array([0.02] * 3 + [1.0] * 3)
    priors[:, 3:] *= np.where(wide, WIDE_ANGLE, 0.01)[:, None]
    pool = LAMBDA_CLASSES if (w >= 24 and h >= 20) else DEFINITE_CLASSES
    classes = [str(rs.choice(pool)) for _ in range(n)]
    exponents = rs.uniform(-2.0, 1.0, n)
    spreads = rs.uniform(-3.0, 3.0, (n, 6))
    full_seeds = rs.randint(0, 2 ** 31 - 1, n)
    scales = [float(rs.choice(LEVEL_SCALES)) for _ in range(nl)]
    lam = [float(v) for v in rs.uniform(0.5, 1.0, nl)]
    mi = [int(v) for v in rs.randint(2, 7, nl)]
    thresholds = bool(rs.randint(0, 3) == 0)
    return dict(index=i, w=w, h=h, nl=nl, holes=holes, fy=fy, n=n, inits=inits, wide=wide, priors=priors, classes=classes,
                exponents=exponents, spreads=spreads, full_seeds=full_seeds, scales=scales, lam=lam, mi=mi,
                thresholds=thresholds)


def information(kind, weight, spread, full_seed):
    if kind == "zero":
        return np.zeros((6, 6))
    if kind == "iso":
        return cases.lambda_iso(weight)
    if kind == "full":
        return cases.lambda_full(int(full_seed), weight)
    if kind == "rotation_only":
        return np.diag(weight * np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]))
    if kind == "translation_only":
        return np.diag(weight * np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]))
    if kind == "diagonal":
        return np.diag(weight * 10.0 ** spread)
    raise KeyError(kind)


def cpu_pyramid(p, nl):
    h, w = p["gray0"].shape
    even = w % 2 ** (nl - 1) == 0 and h % 2 ** (nl - 1) == 0 and nl > 1
    return ie.twin_pyramid(p, nl) if even else ie.oracle_pyramid(p, nl)


@functools.lru_cache(maxsize=None)
def problem(i):
    """Case i in full: the draw, the pair, K, the CPU pyramid, the information matrices and the thresholds."""
    d = dict(draw(i))
    p = synthetic.make_pair(5000 + i, d["w"], d["h"], holes=d["holes"], trans=0.01, rot=0.005)
    K = cases.with_fy(p["K"], d["fy"])
    pyr = cpu_pyramid(p, d["nl"])
    h00 = float(ir.system(pyr[0], 0, K, np.eye(3), np.zeros(3))[1][0, 0])
    weights = h00 * 10.0 ** d["exponents"]
    Lams = np.stack([information(d["classes"][k], weights[k], d["spreads"][k], d["full_seeds"][k]) for k in range(d["n"])])
    mg = [0.0] * d["nl"]
    if d["thresholds"]:
        for L in range(d["nl"] - 1, -1, -1):                   # coarse to fine: the levels above run under their thresholds
            mi = [d["mi"][l] if l > L else (1 if l == L else 0) for l in range(d["nl"])]
            first = pr.optimize(pyr, K, cases.cfg(mi, mg, lam=d["lam"]), d["priors"][0], Lams[0], d["scales"],
                                init_pose=d["inits"][0])
            g = first["gradient_norm"]
            mg[L] = 0.3 * g if np.isfinite(g) else 0.0
    d.update(p=p, K=K, pyr=pyr, h00=h00, Lambdas=Lams, mg=mg)
    return d


def no_prior(d, k):
    """Does pair k of the case run without any prior: Lambda = 0, or every level's scale 0?"""
    return d["classes"][k] == "zero" or not any(d["scales"])


def reference(d, pyr, k, robust):
    """The checker's record of pair k on the given planes."""
    return pr.optimize(pyr, d["K"], cases.cfg(d["mi"], d["mg"], lam=d["lam"]), d["priors"][k], d["Lambdas"][k], d["scales"],
                       robust=robust, init_pose=d["inits"][k])


def set_aside(ref, robust):
    """None, or why the device is not compared with this record -- on the checker's evidence alone."""
    if not (ref["cond"] <= COND_CAP):
        return "cond"
    if ref["margin"] < cases.MARGIN_FLOOR:
        return "threshold margin"
    if robust and ref["bin_margin"] < rcases.BIN_MARGIN_FLOOR:
        return "bin margin"
    if robust and ref["delta_margin"] < rcases.DELTA_MARGIN_FLOOR:
        return "delta margin"
    if not ref["max_angle"] < cases.MAX_PRIOR_ANGLE:
        return "prior angle"
    if not ie.clear_of_the_cuts(ref["state"]):
        return "atan2 keep-out"
    return None
