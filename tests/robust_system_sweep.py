"""The draws of the randomised sweep of phovo_engine_evaluate_robust_pairs (tests/test_gpu_robust_system_sweep.py on the
device, tests/test_robust_system_cpu.py for the draws alone).  Test infrastructure, not collected as tests.

A case is a draw of tests/inverse_system_sweep.py (seed 7: sizes 1..64 x 1..48, perturbed intrinsics, bad source depth, a
depth range sometimes changed, pairs of every frame order, 1, 3 or 40 states) with, from a generator of its own so that those
draws stay what they are, a scale factor (the default, 0.5 or 1.0) and, for three cases in ten, "deltas given": the call
then gets, per pair, `share` (0.3 .. 3) times the threshold the checker computes on the planes the device holds (0.01 where
the pair has no rows).  A case is set aside when it is a knife-edge (one ulp of fx changes the checker's own row count) or
when one of its states comes within the margins on which exact counts rest (1e-7 bins, 1e-10 in |r| - delta): at most
SET_ASIDE_CAP of the cases."""
import numpy as np

import inverse_system_sweep as sw
import robust_system_ref as rsr
from inverse_system_sweep import CASES, FRAME_PAIRS, SEED, SET_ASIDE_CAP, UPLOAD_RANGE, oracle_planes, pair_planes  # noqa: F401

from robust_system_cases import SCALES

OWN_SEED = 1007                         # the generator of this sweep's own draws
GIVEN_SHARE = 0.3
NO_ROWS_DELTA = 0.01
COND_BAR = sw.COND_BAR


def draw_cases(cases=CASES, seed=SEED):
    out = sw.draw_cases(cases, seed)
    rs = np.random.RandomState(OWN_SEED)
    for c in out:
        c["scale"] = float(SCALES[int(rs.randint(len(SCALES)))])
        c["given"] = bool(rs.rand() < GIVEN_SHARE)
        c["share"] = rs.uniform(0.3, 3.0, len(c["states"]))
    return out


def given_deltas(c, frames):
    """The deltas of a "deltas given" case, from the checker on the per-frame planes `frames`; None for the others."""
    if not c["given"]:
        return None
    out = np.empty(len(c["states"]))
    for k, st in enumerate(c["states"]):
        own = rsr.system(pair_planes(frames, c["orders"][k]), 0, c["K"], st, c["scale"], c["lo"], c["hi"])["delta"]
        out[k] = c["share"][k] * own if own > 0.0 and np.isfinite(own) else NO_ROWS_DELTA
    return out


def references(c, frames):
    """The checker's records of the case's pairs on the per-frame planes `frames`, the deltas the call is given (or None),
    and why the case is set aside ("" if it is not)."""
    deltas = given_deltas(c, frames)
    refs = [rsr.system(pair_planes(frames, c["orders"][k]), 0, c["K"], c["states"][k], c["scale"], c["lo"], c["hi"],
                       None if deltas is None else deltas[k]) for k in range(len(c["states"]))]
    _, knife = sw.references(c, frames)
    if knife:
        return refs, deltas, "one ulp of fx changes the checker's row count"
    for k, ref in enumerate(refs):
        if not rsr.margins_hold(ref):
            return refs, deltas, f"state {k}: bin margin {ref['bin_margin']:.3g}, delta margin {ref['delta_margin']:.3g}"
    return refs, deltas, ""


def relative_bars_apply(ref):
    """False: the record is compared on counts, delta, flags and costs only (fewer than 6 rows, a non-finite sum, or cond(H)
    above 1e8)."""
    H, g = ref["H"], ref["g"]
    if ref["rows"] < 6 or not np.all(np.isfinite(H)) or not np.all(np.isfinite(g)):
        return False
    with np.errstate(all="ignore"):
        return bool(np.linalg.cond(H) <= COND_BAR)


def classes_seen(cases):
    seen = sw.classes_seen(cases)
    seen["scale"] = sorted({c["scale"] for c in cases})
    seen["given"] = sorted({c["given"] for c in cases})
    return seen
