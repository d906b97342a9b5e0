"""The fixtures of tests/test_gpu_geometric.py, in one place so that tests/test_geometric_cpu.py can pre-check every one of
them with the checker alone (cond, threshold margin, gate margin) before a device sees it.  Not collected as a test.

A case is dict(pair, nl, mi, mg, lam, weight, limit, init, K): a frame pair of photoconsistency synthetic data, the level
loop's settings, the per-level depth weight and residual limit (<= 0: gate off) and the start pose (default: START, below)."""
import os

import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import native, synthetic
from oracle import numpy_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED_4_LEVEL = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")

# one level; (w, h): exactly one 64-pixel chunk, less than a chunk, the two strips (clamp bands on every row; no gradient
# across the strip, so the system is exactly singular on both sides), a partial last chunk over several waves, 80x60
SHAPES = [(8, 8), (7, 5), (45, 1), (1, 45), (75, 53), (80, 60)]
STRIPS = {(45, 1), (1, 45)}
# the residual gate where it is on: tight enough to drop rows of a pair that starts 1 cm and 5 mrad away from its answer.
# Depths lie on a 1 mm grid and a zero start warps every pixel onto itself, so the first residuals are whole millimetres:
# every limit below lies off that grid (and off the quarter-millimetre grid of level 1), or a fixture would sit exactly on
# its gate.
TIGHT_GATE = 0.0045


# The start pose of every fixture that is compared with the checker: small, and NOT zero.  From a zero start every source
# pixel warps onto its own centre up to rounding, and the last bit of u decides which cell's taps and which one-sided depth
# derivative a row takes -- on the device and in the checker independently (geometric_ref.rows_vectorised, cell_margin).
START = np.array([1.3e-3, -0.7e-3, 0.9e-3, 0.6e-3, -0.8e-3, 0.5e-3])
# ... and the least distance from a pixel centre a fixture's rows must keep: u and v are O(100) and carry a few roundings
# (1e-13), so 1e-9 pixels is four orders above what the two sides can disagree by
CELL_FLOOR = 1e-9


def _case(pair, nl, mi, mg=None, lam=None, weight=1.0, limit=0.0, init=START, K=None):
    as_list = lambda v: [float(v)] * nl if np.isscalar(v) else [float(x) for x in v]
    return dict(pair=pair, nl=nl, mi=list(mi), mg=as_list(0.0 if mg is None else mg), lam=as_list(1.0 if lam is None else lam),
                weight=as_list(weight), limit=as_list(limit), init=init, K=pair["K"] if K is None else K)


def shape_case(w, h, gate):
    p = synthetic.make_pair(1, w, h, holes=0.02, trans=0.01, rot=0.005)
    return _case(p, 1, [5], limit=TIGHT_GATE if gate else 0.0)


def two_level_case(gate):
    return _case(synthetic.make_pair(2, 150, 100, holes=0.02), 2, [5, 5], limit=0.0106 if gate else 0.0)


def holes_pair(seed=12, w=80, h=60):
    """Target depth with NaN, 0 and beyond-max holes (5 % each), on top of the i.i.d. holes of both frames."""
    p = synthetic.make_pair(seed, w, h, holes=0.02)
    rs = np.random.RandomState(77)
    u = rs.uniform(size=p["depth1"].shape)
    d1 = p["depth1"].astype(np.float64).copy()
    d1[u < 0.05] = np.nan
    d1[(u >= 0.05) & (u < 0.10)] = 0.0
    d1[(u >= 0.10) & (u < 0.15)] = 7.0
    p["depth1"] = d1
    return p


def skewed_intrinsics_case():
    p = synthetic.make_pair(13, 80, 60, holes=0.02)
    K = p["K"].copy()
    K[1, 1] *= 1.1            # fy != fx
    K[0, 2] += 3.3            # a moved principal point
    K[1, 2] -= 2.7
    return _case(p, 2, [4, 4], weight=2.0, limit=0.0505, K=K)


def shipped_case(fixed):
    n = native.read_config_file(SHIPPED_4_LEVEL)
    nl = n.num_levels
    mi = list(n.max_num_iterations[:nl])
    mg = [0.0] * nl if fixed else list(n.min_gradient_norm[:nl])
    return _case(synthetic.make_pair(21, 640, 480, holes=0.02), nl, mi, mg=mg, weight=3.0, limit=0.1)


def all_invalid_target_case():
    p = synthetic.make_pair(14, 80, 60, holes=0.02)
    p["depth1"] = np.zeros_like(p["depth1"])
    return _case(p, 2, [5, 5], weight=3.0, limit=0.1)


def all_nan_source_case():
    p = synthetic.make_pair(7, 80, 60)
    p["depth0"] = np.full_like(p["depth0"], np.nan)
    return _case(p, 2, [4, 4])


def nonzero_start_case():
    p = synthetic.make_pair(15, 80, 60, holes=0.02)
    return _case(p, 2, [5, 5], weight=3.0, limit=0.0505, init=0.5 * p["motion"])


CASES = {}
for _w, _h in SHAPES:
    for _gate in (False, True):
        CASES[f"{_w}x{_h}-{'gate' if _gate else 'nogate'}"] = (lambda w=_w, h=_h, g=_gate: shape_case(w, h, g))
CASES.update({
    "two-levels-nogate": lambda: two_level_case(False),
    "two-levels-gate": lambda: two_level_case(True),
    "per-level-weights": lambda: _case(synthetic.make_pair(3, 150, 100, holes=0.02), 2, [5, 5], weight=[0.5, 4.0],
                                       limit=[0.0213, 0.0]),
    "skewed-intrinsics": skewed_intrinsics_case,
    "lambda": lambda: _case(synthetic.make_pair(11, 80, 60, holes=0.02), 2, [5, 5], lam=[0.7, 0.5], weight=3.0, limit=0.1),
    "nonzero-start": nonzero_start_case,
    "target-holes": lambda: _case(holes_pair(), 2, [5, 5], weight=3.0, limit=0.1),
    "all-invalid-target": all_invalid_target_case,
    "all-nan-source": all_nan_source_case,
    "shipped": lambda: shipped_case(False),
    "shipped-fixed": lambda: shipped_case(True),
})
# cases whose system is singular BY CONSTRUCTION, exactly, on the device and in the checker alike (an exact zero column, or
# no row at all): no pose bar applies to them, and the pre-check asserts that instead of cond <= 1e5
SINGULAR = {f"{w}x{h}-{g}" for (w, h) in STRIPS for g in ("gate", "nogate")} | {"all-nan-source"}

# plane-scene 160x120 pairs for the ground-truth test (sigma = 3, gate 0.1 m, 3 levels of 10 iterations): only seeds for which
# tests/test_geometric_cpu.py asserts that the checker is at least 2x closer to `motion` than the bilinear-corrected
# photometric checker
GROUND_TRUTH_SEEDS = (2, 3, 5, 6)
GROUND_TRUTH = dict(nl=3, mi=[10, 10, 10], weight=3.0, limit=0.1)


def ground_truth_case(seed):
    g = GROUND_TRUTH
    return _case(synthetic.make_pair(seed, 160, 120), g["nl"], g["mi"], weight=g["weight"], limit=g["limit"], init=None)


def checker_cfg(case):
    return dict(num_levels=case["nl"], lam=case["lam"], max_iter=case["mi"], min_grad=case["mg"],
                depth_weight=case["weight"], max_depth_residual=case["limit"])


def twin_pyramid(case):
    """pyr[L] = (i0, d0, i1, gx1, gy1, d1) from the numpy twin's pyramid producers with the library's default gradient
    scale (None on levels the case does not optimise)."""
    p, nl = case["pair"], case["nl"]
    scale = list(native.make_config(num_levels=nl).image_gradients_scaling_factor[:nl])
    base = twin.build_pyramids(p["gray0"], p["depth0"], p["gray1"], nl, scale)
    d1 = np.asarray(p["depth1"], dtype=np.float64)
    return [base[l] + (twin.resize_level(d1, l),) if case["mi"][l] > 0 else None for l in range(nl)]
