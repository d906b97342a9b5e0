"""The draws of the randomised sweep of phovo_engine_evaluate_objective_pairs (tests/test_gpu_objective_system_sweep.py on
the device, tests/test_objective_system_cpu.py for the draws alone).  Test infrastructure, not collected as tests.

A case is one one-level problem of 1..64 x 1..48 pixels (strips included) with perturbed intrinsics, one kind of bad source
depth, a depth range that is sometimes changed between the upload and the call, and 1, 3 or 40 states around the pair's
motion or from edge_states.  A case is set aside only when it is a knife-edge: when one ulp of fx changes the checker's own
row count for one of its states."""
import numpy as np

import edge_states
import objective_system_ref as osr

import phovo_amd  # noqa: F401
from phovo_amd import synthetic

CASES = 200
SEED = 22                               # the checkers alone set no case of it aside (tests/test_objective_system_cpu.py)
DEPTH_KINDS = ("clean", "nan", "inf", "at_min", "at_max")
SIZE_CLASSES = ("strip", "tile1", "tiles2", "tiles3")
UPLOAD_RANGE = (0.3, 5.0)
CALL_RANGE = (0.5, 3.0)                 # the range in force at the call in the cases that change it
COND_BAR = 1e8
SET_ASIDE_CAP = 0.02
_EDGE = None


def size_class(w, h):
    if w < 8 or h < 8:
        return "strip"
    return ("tile1", "tiles2", "tiles3")[(w * h - 1) // 1024]


def draw_case(rs):
    global _EDGE
    if _EDGE is None:
        _EDGE = np.array(edge_states.initial_states())
    w, h = int(rs.randint(1, 65)), int(rs.randint(1, 49))
    seed = int(rs.randint(0, 1 << 20))
    p = synthetic.make_pair(seed, w if w >= 8 else 64, h, holes=0.02)
    if w < 8:                                                    # a narrow strip of a wider render
        for k in ("gray0", "depth0", "gray1", "depth1"):
            p[k] = np.ascontiguousarray(p[k][:, 30:30 + w])
    K = np.array(p["K"], dtype=np.float64)
    K[0, 0] *= rs.uniform(0.9, 1.1)
    K[1, 1] *= rs.uniform(0.9, 1.1)
    K[0, 2] += rs.uniform(-1.5, 1.5)
    K[1, 2] += rs.uniform(-1.5, 1.5)
    kind = DEPTH_KINDS[int(rs.randint(len(DEPTH_KINDS)))]
    changed = bool(rs.rand() < 0.3)
    lo, hi = CALL_RANGE if changed else UPLOAD_RANGE
    d0 = p["depth0"].copy()
    bad = dict(clean=None, nan=np.nan, inf=np.inf, at_min=lo, at_max=hi)[kind]
    if bad is not None:
        d0[int(rs.randint(h)), :] = bad
        d0[:, int(rs.randint(w))] = bad
    n_pairs = int((1, 3, 40)[int(rs.choice(3, p=[0.45, 0.45, 0.1]))])
    motion = np.asarray(p["motion"], dtype=np.float64)
    states = motion + rs.uniform(-0.02, 0.02, (n_pairs, 6))
    for k in range(n_pairs):
        if rs.rand() < 0.1:
            states[k] = _EDGE[int(rs.randint(len(_EDGE)))]
    return dict(w=w, h=h, K=K, gray0=p["gray0"], depth0=d0, gray1=p["gray1"], depth1=p["depth1"], kind=kind, changed=changed,
                lo=lo, hi=hi, states=states, size_class=size_class(w, h))


def draw_cases(cases=CASES, seed=SEED):
    rs = np.random.RandomState(seed)
    return [draw_case(rs) for _ in range(cases)]


def oracle_planes(c):
    """The case's planes from the oracle's pyramid functions (depth gradients with the max depth in force at upload)."""
    return osr.oracle_planes(dict(gray0=c["gray0"], depth0=c["depth0"], gray1=c["gray1"], depth1=c["depth1"]), UPLOAD_RANGE[1])


def _fx_neighbours(K):
    out = []
    for to in (-np.inf, np.inf):
        K2 = np.array(K, dtype=np.float64)
        K2[0, 0] = np.nextafter(K2[0, 0], to)
        out.append(K2)
    return out


def references(c, pl, which):
    """The checker's systems of the case's states on planes `pl` (which: "tr" or "bi"), and whether the case is a
    knife-edge: one ulp of fx changes the checker's own row count of some state."""
    def one(K, st):
        if which == "tr":
            return osr.trust_region_system(pl["i0"], pl["d0"], pl["i1"], pl["gx"], pl["gy"], 0, K, st, c["lo"], c["hi"])
        return osr.biobjective_system(pl["i0"], pl["d0"], pl["i1"], pl["d1"], pl["gx"], pl["gy"], pl["dgx"], pl["dgy"],
                                      pl["gain"], 0, K, st, c["lo"], c["hi"])
    refs = [one(c["K"], st) for st in c["states"]]
    knife = any(one(K2, st)["rows"] != r["rows"] for K2 in _fx_neighbours(c["K"]) for st, r in zip(c["states"], refs))
    return refs, knife


def relative_bars_apply(ref):
    """False: the case is compared on rows, flags and cost only (fewer than 6 rows, or cond(J^T J) above 1e8)."""
    return ref["rows"] >= 6 and osr.cond(ref["H"]) <= COND_BAR
