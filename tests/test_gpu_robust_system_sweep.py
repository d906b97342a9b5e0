"""Randomised sweep of phovo_engine_evaluate_robust_pairs on the device (-m gpu): the 200 draws of
tests/robust_system_sweep.py -- those of tests/inverse_system_sweep.py (sizes 1..64 x 1..48 with strips, perturbed
intrinsics, NaN / inf source depth and depth exactly at the gate's bounds, a depth range sometimes changed between upload and
call, three frames paired in every order, states around zero and from edge_states, 1, 3 or 40 pairs) with a drawn scale
factor and, for three cases in ten, deltas given -- against the checker fed the planes as the device holds them.  A case is
set aside only as a knife-edge (one ulp of fx changes the checker's own row count) or for a margin (an |r| within 1e-7 bins
of a bin's edge or within 1e-10 of its delta), at most 2 % of them, each printed with its reason; records with fewer than 6
rows, a non-finite sum or cond(H) above 1e8 are compared on counts, delta, flags and costs only.  Failures allowed: 0."""
import numpy as np
import pytest

import robust_system_ref as rsr
import robust_system_sweep as sw

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

pytestmark = pytest.mark.gpu


def _check(rec, k, ref, relative, given):
    if relative:
        return rsr.check_record(rec, k, ref, given)
    assert rec["rows"][k] == ref["rows"], (rec["rows"][k], ref["rows"])
    assert rec["outliers"][k] == ref["outliers"], (rec["outliers"][k], ref["outliers"])
    assert rec["flags"][k] == rsr.flags_of(ref), (rec["flags"][k], rsr.flags_of(ref))
    if given:
        assert rec["delta"][k] == ref["delta"] and rec["median"][k] == 0.0
    else:
        assert rsr.ulps(rec["delta"][k], ref["delta"]) <= rsr.ULPS and rsr.ulps(rec["median"][k], ref["median"]) <= rsr.ULPS
    for c in rsr.COSTS:
        if np.isfinite(ref[c]):
            assert abs(rec[c][k] - ref[c]) <= rsr.COST_BAR * abs(ref[c]), (c, rec[c][k], ref[c])
        else:
            assert not np.isfinite(rec[c][k]), c
    return 0.0, 0.0


def test_sweep_against_checker():
    cases = sw.draw_cases()
    set_aside, compared, weak, worst = 0, 0, 0, (0.0, 0.0)
    for ci, c in enumerate(cases):
        with odometry.AlignmentEngine(0) as e:
            e.set_config(native.make_config(num_levels=1, max_iter=[1], min_grad=[0.0]))
            e.set_objective(native.OBJECTIVE_INVERSE_ROBUST)
            e.set_robust_options(native.make_robust_options(c["scale"]))
            e.set_intrinsic_matrix(c["K"])
            e.set_depth_range(*sw.UPLOAD_RANGE)
            e.reserve_frames(3, c["w"], c["h"])
            e.upload_frames(0, c["gray"], c["depth"])
            if c["changed"]:
                e.set_depth_range(c["lo"], c["hi"])
            frames = [e.get_level_planes(f, 0) for f in range(3)]
            refs, deltas, why = sw.references(c, frames)          # (the given deltas come from the checker on these planes)
            src = [sw.FRAME_PAIRS[o][0] for o in c["orders"]]
            tgt = [sw.FRAME_PAIRS[o][1] for o in c["orders"]]
            rec = e.evaluate_robust_pairs(src, tgt, c["states"], 0, deltas=deltas)
        if why:
            set_aside += 1
            print(f"set aside: case {ci} ({c['w']}x{c['h']}, {c['kind']}): {why}")
            continue
        for k, ref in enumerate(refs):
            relative = sw.relative_bars_apply(ref)
            weak += not relative
            compared += 1
            try:
                dh, dg = _check(rec, k, ref, relative, c["given"])
            except AssertionError as err:
                raise AssertionError(f"case {ci} ({c['w']}x{c['h']}, {c['kind']}, range changed: {c['changed']}, scale "
                                     f"{c['scale']}, deltas given: {c['given']}), state {k} ({c['orders'][k]}): {err}") from err
            worst = (max(worst[0], dh), max(worst[1], dg))
    print("cases", len(cases), "set aside", set_aside, "records compared", compared, "on counts and costs only", weak,
          f"worst dH / bar {worst[0]:.3g}, dg / bar {worst[1]:.3g}")
    assert set_aside <= sw.SET_ASIDE_CAP * len(cases)
