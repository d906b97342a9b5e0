"""The randomised sweep of the photometric-geometric kernels (gn_geometric_kernel.hip, DESIGN.md §16;
gn_evaluate_geometric_kernels.hip, §17) on the device: the 64 seeded cases of tests/geometric_sweep.py, eight per test.  Each
case is aligned (three copies, bit-identical) and held to geometric_ref.optimize on the planes the device holds, under
test_gpu_geometric._compare's bars (cond(H) above 1e5 widens pose_bar, it does not set a case aside; a case that ends
non-finite is compared on counts, flags and the iteration it ended at); then the same case goes through
evaluate_geometric_pairs at its start pose and at the checker's final pose on every level, against
geometric_system_ref.blocks under check_record's bars.  A case is set aside only for a margin (geometric_sweep.judge), and
at most MAX_SKIPPED of the 64 may be; tests/test_geometric_sweep_cpu.py holds the checker alone to the same cap."""
import numpy as np
import pytest

import phovo_amd  # noqa: F401

import geometric_edges as ge
import geometric_sweep as gs
from test_gpu_geometric import _device_pyramid
from test_gpu_geometric_edges import _align, _hold, _hold_system, _open, _three_alike

pytestmark = pytest.mark.gpu

_DONE = {}                                # seed -> why the case was set aside (None: compared), filled once per case


def _run(seed):
    if seed in _DONE:
        return _DONE[seed]
    case = gs.draw_case(seed)
    p, K = gs.pair_of(case)
    c = gs.checker_cfg(case)
    nl = case["nl"]
    with _open(p, K, c) as eng:
        pyr = _device_pyramid(eng, 0, 1, nl, case["mi"])
        s, reps, g = _align(eng, [0] * 3, [1] * 3, np.tile(case["init"], (3, 1)))
        j = gs.judge(case, pyr, K)
        recs = {level: eng.evaluate_geometric_pairs([0, 0], [1, 1], j["states"], level) for level in range(nl)}
    _three_alike(s, reps, g, nl)
    what = f"seed {seed} {case['w']}x{case['h']} levels {nl} range {case['depth_range']}"
    _DONE[seed] = j["skip"]
    if j["skip"] is not None:
        print(f"{what}: set aside ({j['skip']})")
        return j["skip"]
    _hold("H", what, s[0], reps[0], g[0], j["ref"], nl, expect_flat=ge.flat(j["ref"]))
    for (level, which), ref in j["blocks"].items():
        _hold_system("H", f"{what} level {level} at {'start' if which == 0 else 'end'}", recs[level][which], ref)
    return None


@pytest.mark.parametrize("group", range(len(gs.GROUPS)))
def test_geometric_randomised_sweep_against_the_checkers(group):
    for seed in gs.GROUPS[group]:
        _run(seed)


def test_geometric_sweep_sets_aside_no_more_than_the_cap():
    """On the device's planes, as on the CPU pyramids: at most MAX_SKIPPED of the 64 cases are set aside."""
    skipped = [seed for seed in gs.SEEDS if _run(seed) is not None]
    print(f"set aside: {skipped}")
    assert len(gs.SEEDS) == gs.N_CASES and len(skipped) <= gs.MAX_SKIPPED, skipped
