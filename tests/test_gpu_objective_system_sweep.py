"""Randomised sweep of phovo_engine_evaluate_objective_pairs on the device (-m gpu): the 200 draws of
tests/objective_system_sweep.py per objective -- sizes 1..64 x 1..48 with strips, perturbed intrinsics, NaN / inf source
depth and depth exactly at the gate's bounds, a depth range sometimes changed between upload and call, states around the
motion and from edge_states, 1, 3 or 40 pairs -- against the checker fed the planes as the device holds them.  A case is
set aside only as a knife-edge (one ulp of fx changes the checker's own row count), at most 2 % of them; cases with fewer
than 6 rows or cond(J^T J) above 1e8 are compared on rows, flags and cost only."""
import numpy as np
import pytest

import objective_system_ref as osr
import objective_system_sweep as sw

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return sw.draw_cases()


@pytest.mark.parametrize("which,objective", [("tr", native.OBJECTIVE_TRUST_REGION), ("bi", native.OBJECTIVE_BIOBJECTIVE)],
                         ids=["trust_region", "biobjective"])
def test_sweep_against_checker(cases, which, objective):
    set_aside, compared, weak = 0, 0, 0
    for ci, c in enumerate(cases):
        n = len(c["states"])
        with odometry.AlignmentEngine(0) as e:
            e.set_config(native.make_config(num_levels=1, max_iter=[1], min_grad=[0.0]))
            e.set_intrinsic_matrix(c["K"])
            e.set_objective(objective)
            e.set_depth_range(*sw.UPLOAD_RANGE)
            e.reserve_frames(2, c["w"], c["h"])
            e.upload_frame(0, c["gray0"], c["depth0"])
            e.upload_frame(1, c["gray1"], c["depth1"])
            if c["changed"]:
                e.set_depth_range(c["lo"], c["hi"])
            i0, d0, _, _ = e.get_level_planes(0, 0)
            i1, d1, gx, gy = e.get_level_planes(1, 0)
            pl = dict(i0=i0, d0=d0, i1=i1, d1=d1, gx=gx, gy=gy)
            if which == "bi":
                pl["dgx"], pl["dgy"] = e.get_level_depth_gradients(1, 0)
                pl["gain"] = e.get_level_depth_gain(1, 0)
            rec = e.evaluate_objective_pairs([0] * n, [1] * n, c["states"], 0)
        refs, knife = sw.references(c, pl, which)
        if knife:
            set_aside += 1
            continue
        for k, ref in enumerate(refs):
            relative = sw.relative_bars_apply(ref)
            weak += not relative
            compared += 1
            try:
                osr.check_record(rec, k, ref, relative=relative)
            except AssertionError as err:
                raise AssertionError(f"case {ci} ({c['w']}x{c['h']}, {c['kind']}, range changed: {c['changed']}), "
                                     f"state {k}: {err}") from err
    print(which, "cases", len(cases), "set aside", set_aside, "records compared", compared, "on rows/flags/cost only", weak)
    assert set_aside <= sw.SET_ASIDE_CAP * len(cases)
