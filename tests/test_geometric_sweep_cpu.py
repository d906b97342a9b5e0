"""CPU side of the photometric-geometric kernels' randomised sweep (tests/geometric_sweep.py; tests/test_gpu_geometric_sweep.py
walks the same seeds on the device).  With the checkers alone, on pyramids built by the oracle's producers:
the committed seeds reach every size, level count, depth range and gate setting; at most MAX_SKIPPED cases are set aside for
a margin, so the cap cannot be filled by inputs on which the checker itself is undecided; most cases are held to the flat
bar and have depth rows on every level (the tally is printed: with the committed seeds none is set aside, all 64 end
finite under the flat bar).  No GPU."""
import collections

import numpy as np
import pytest

import geometric_edges as ge
import geometric_ref as gr
import geometric_sweep as gs


def test_the_seed_list_is_fixed_and_the_draws_are_reproducible():
    assert gs.SEEDS == list(range(2000, 2064)) and [len(g) for g in gs.GROUPS] == [8] * 8
    a, b = gs.draw_case(gs.SEEDS[5]), gs.draw_case(gs.SEEDS[5])
    assert repr(a) == repr(b)
    for seed in gs.SEEDS:
        c = gs.draw_case(seed)
        assert (c["w"], c["h"]) in gs.SIZES and c["nl"] in (1, 2) and c["depth_range"] in gs.RANGES
        assert c["nl"] == 1 or (c["w"], c["h"]) in gs.HALVES_CLEANLY
        assert all(0.25 <= s <= 8.0 for s in c["weight"]) and all(0.5 <= l <= 1.0 for l in c["lam"])
        assert all(1 <= m <= 6 for m in c["mi"]) and 0.9 <= c["fy_over_fx"] <= 1.1 and max(np.abs(c["shift"])) <= 0.45
        assert all(l == 0.0 or (l * 1000.0) % 1.0 != 0.0 for l in c["limit"])            # off the millimetre grid
        assert np.all(np.abs(c["init"] - ge.START) <= gs.START_SCALE) and np.all(c["init"] != 0.0)


def test_the_committed_seeds_reach_every_class():
    cov = gs.coverage([gs.draw_case(s) for s in gs.SEEDS])
    print(cov)
    want = [f"size_{w}x{h}" for w, h in gs.SIZES] + ["levels_1", "levels_2", "gate_on", "gate_off"]
    want += [f"range_{lo}" for lo, _ in gs.RANGES]
    for key in want:
        assert cov.get(key, 0) >= 4, (key, cov)


@pytest.fixture(scope="module")
def judged():
    out = []
    for seed in gs.SEEDS:
        case = gs.draw_case(seed)
        pyr, K = gs.cpu_pyramid(case)
        out.append((case, gs.judge(case, pyr, K)))
    return out


def test_the_checker_alone_stays_inside_the_skip_cap(judged):
    tally = collections.Counter()
    for case, j in judged:
        ref = j["ref"]
        finite = bool(np.all(np.isfinite(ref["state"])))
        tally["skipped"] += j["skip"] is not None
        tally["finite"] += finite
        tally["nonfinite"] += not finite
        tally["flat"] += finite and ge.flat(ref)
        tally["rank_deficient"] += bool(ref["flags"] & gr.PAIR_RANK_DEFICIENT)
        tally["depth_rows"] += min(ref["depth_rows"]) > 0
        if j["skip"]:
            print(case["seed"], j["skip"])
    print(dict(tally))
    assert tally["skipped"] <= gs.MAX_SKIPPED, tally
    assert tally["flat"] >= 2 * gs.N_CASES // 3, tally        # most cases are held to the flat bar
    assert tally["depth_rows"] >= gs.N_CASES // 2, tally      # ... and have depth rows on every level


def test_the_evaluate_states_have_rows(judged):
    """The second half of the sweep is not vacuous: most (case, level, state) systems have depth rows."""
    with_rows = total = 0
    for case, j in judged:
        for b in j["blocks"].values():
            total += 1
            with_rows += b["depth_rows"] > 6
    print(with_rows, total)
    assert with_rows >= 2 * total // 3
