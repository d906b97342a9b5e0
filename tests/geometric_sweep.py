"""The randomised sweep of the photometric-geometric kernels: a seeded generator of small cases, one per
seed of SEEDS, walked by tests/test_geometric_sweep_cpu.py with the checkers alone (on pyramids built by the oracle's
producers) and by tests/test_gpu_geometric_sweep.py on the device (the checkers on the planes read back from it).  Test
infrastructure, not collected.

A case draws: the size, 1 or 2 levels (2 only where the size halves cleanly), a synthetic.make_pair scene with its own
motion and holes, NaN / 0 / beyond-max holes in the target depth (geometric_cases.holes_pair's kinds), fy / fx, a shift of
the principal point, the depth range, the depth weight (log-uniform), the residual limit (off, or a value off the
millimetre grid), lambda, the iteration counts and a start pose near geometric_cases.START.

judge() runs the checkers on a pyramid and says whether the case is compared or set aside.  A case is set aside only when
the checker's own run -- or one of the evaluate call's states -- comes closer than 1e-6 relative to a residual gate or a
gradient threshold or closer than CELL_FLOOR to a pixel centre: there the device and the checker may take different rows by
the last bit.  At most MAX_SKIPPED of the cases may be.  A large cond(H) is no reason (pose_bar widens), nor
is a state that goes non-finite (counts, flags and the iteration it ended at are compared)."""
import numpy as np

import phovo_amd  # noqa: F401
from phovo_amd import synthetic

import geometric_cases as gc
import geometric_edges as ge
import geometric_ref as gr
import geometric_system_ref as gsr

BASE_SEED = 2000
N_CASES, GROUP, MAX_SKIPPED = 64, 8, 4
SEEDS = [BASE_SEED + i for i in range(N_CASES)]
GROUPS = [SEEDS[i:i + GROUP] for i in range(0, N_CASES, GROUP)]

SIZES = ((7, 5), (24, 20), (33, 17), (48, 36), (75, 53))
HALVES_CLEANLY = {(24, 20), (48, 36)}
RANGES = ((0.3, 5.0), (0.5, 3.0), (1.0, 2.5))
LIMITS = (0.0, 0.0045, 0.0213, 0.0505, 0.1)      # 0: the gate is off
BEYOND_MAX = 7.0                                 # beyond every range's max_depth
START_SCALE = np.array([0.01, 0.01, 0.01, 0.005, 0.005, 0.005])


def draw_case(seed):
    rs = np.random.RandomState(seed)
    w, h = SIZES[rs.randint(len(SIZES))]
    nl = int(rs.randint(1, 3)) if (w, h) in HALVES_CLEANLY else 1
    case = dict(seed=seed, w=w, h=h, nl=nl,
                pair_seed=int(rs.randint(1, 10000)), trans=float(rs.uniform(0.0, 0.03)), rot=float(rs.uniform(0.0, 0.02)),
                holes=float(rs.uniform(0.0, 0.1)), target_holes=float(rs.uniform(0.0, 0.1)), hole_seed=int(rs.randint(1, 10000)),
                fy_over_fx=float(rs.uniform(0.9, 1.1)), shift=[float(v) for v in rs.uniform(-0.45, 0.45, 2)],
                depth_range=RANGES[rs.randint(len(RANGES))],
                weight=[float(np.exp(rs.uniform(np.log(0.25), np.log(8.0)))) for _ in range(nl)])
    limits = []
    for _ in range(nl):
        base = LIMITS[rs.randint(len(LIMITS))]
        limits.append(float(base * (1.0 + rs.uniform(-0.03, 0.03))))          # off the millimetre grid
    case.update(limit=limits, lam=[float(v) for v in rs.uniform(0.5, 1.0, nl)],
                mi=[int(v) for v in rs.randint(1, 7, nl)],
                init=gc.START + rs.uniform(-1.0, 1.0, 6) * START_SCALE)
    return case


def pair_of(case):
    """The frames and K of a case: make_pair's, the target depth with NaN / 0 / beyond-max holes, K perturbed."""
    p = synthetic.make_pair(case["pair_seed"], case["w"], case["h"], holes=case["holes"], trans=case["trans"], rot=case["rot"])
    u = np.random.RandomState(case["hole_seed"]).uniform(size=p["depth1"].shape)
    f = case["target_holes"] / 3.0
    d1 = np.asarray(p["depth1"], dtype=np.float64).copy()
    d1[u < f] = np.nan
    d1[(u >= f) & (u < 2 * f)] = 0.0
    d1[(u >= 2 * f) & (u < 3 * f)] = BEYOND_MAX
    p["depth1"] = d1
    K = p["K"].copy()
    K[1, 1] = case["fy_over_fx"] * K[0, 0]
    K[0, 2] += case["shift"][0]
    K[1, 2] += case["shift"][1]
    return p, K


def checker_cfg(case):
    lo, hi = case["depth_range"]
    return ge.cfg(case["mi"], lam=case["lam"], weight=case["weight"], limit=case["limit"], lo=lo, hi=hi)


def cpu_pyramid(case):
    p, K = pair_of(case)
    return ge.pyramid(p, case["nl"]), K


def judge(case, pyr, K):
    """The checkers on pyr: dict(ref, states, blocks, skip).  states: the start pose and the checker's final pose; blocks[
    (level, which)]: geometric_system_ref.blocks there; skip: None, or why the case is set aside."""
    c = checker_cfg(case)
    ref = gr.optimize(pyr, K, c, case["init"])
    states = np.stack([np.asarray(case["init"], dtype=np.float64), ref["state"]])
    skip = None
    if not ref["margin"] > ge.MARGIN_FLOOR:
        skip = "threshold margin"
    elif not ref["gate_margin"] > ge.MARGIN_FLOOR:
        skip = "gate margin"
    elif not ref["cell_margin"] > gc.CELL_FLOOR:
        skip = "cell margin"
    blocks = {}
    for level in range(case["nl"]):
        for which in range(2):
            b = gsr.blocks(pyr[level], level, K, states[which], c["depth_weight"][level], c["max_depth_residual"][level],
                           c["min_depth"], c["max_depth"])
            blocks[(level, which)] = b
            if skip is None and not (b["cell_margin"] > gc.CELL_FLOOR and b["gate_margin"] > gsr.MARGIN_FLOOR):
                skip = "evaluate margin"
    return dict(ref=ref, states=states, blocks=blocks, skip=skip)


def coverage(cases):
    """What the drawn cases reach: counts per size, level count, range, gate on / off."""
    cov = {}
    for c in cases:
        for key in (f"size_{c['w']}x{c['h']}", f"levels_{c['nl']}", f"range_{c['depth_range'][0]}",
                    "gate_on" if any(l > 0 for l in c["limit"]) else "gate_off"):
            cov[key] = cov.get(key, 0) + 1
    return cov
