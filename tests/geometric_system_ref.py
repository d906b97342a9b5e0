"""CPU checker of phovo_engine_evaluate_geometric_pairs, in numpy: the photometric and the depth block of
the photometric-geometric objective's Gauss-Newton system at a pose on one level, apart.  Built from
geometric_ref.rows_vectorised, so the rows are the aligner's checker's rows; the bars are sampled_system_ref.check_against's
(DESIGN.md §11), applied to the photometric block with its cost, to the depth block with its cost and to the sum with the
summed cost.  Test infrastructure, not collected."""
import numpy as np

import geometric_cases as gc
import geometric_ref as gr
import sampled_system_ref as ssr

MARGIN_FLOOR = 1e-6           # the least relative distance of any row's |D1(u, v) - Z'| from the residual gate
# the fixtures of tests/test_gpu_geometric_system.py: every case of geometric_cases but the 640x480 ones, on every level it
# optimises, at START, at the pair's motion and at the optimum (tests/test_geometric_system_cpu.py pre-checks them all)
CASE_NAMES = [n for n in gc.CASES if not n.startswith("shipped")]
STATE_NAMES = ("start", "motion", "optimum")


def levels_of(case):
    return [l for l in range(case["nl"]) if case["mi"][l] > 0]


def states_of(case, optimum):
    """The three states a fixture is evaluated at; `optimum` is the aligner's (or its checker's) returned state."""
    return dict(start=np.array(gc.START), motion=np.asarray(case["pair"]["motion"], dtype=np.float64),
                optimum=np.asarray(optimum, dtype=np.float64))


def blocks(planes, level, K, pose, sigma, limit, min_depth=0.3, max_depth=5.0):
    """dict(H_I[6,6], g_I[6], H_D[6,6], g_D[6], photometric_cost, depth_cost, rows, depth_rows, gate_margin, cell_margin)
    at the pose; planes = (i0, d0, i1, gx1, gy1, d1) of the level."""
    v = gr.rows_vectorised(planes, level, K, pose, sigma, limit, min_depth, max_depth)
    with np.errstate(all="ignore"):
        rI, JI = v["rI"][v["rows"]], v["JI"][v["rows"]]
        rD, JD = v["rD"][v["drows"]], v["JD"][v["drows"]]
        return dict(H_I=JI.T @ JI, g_I=JI.T @ rI, H_D=JD.T @ JD, g_D=JD.T @ rD,
                    photometric_cost=float(rI @ rI), depth_cost=float(rD @ rD),
                    rows=int(v["rows"].sum()), depth_rows=int(v["drows"].sum()),
                    gate_margin=v["gate_margin"], cell_margin=v["cell_margin"])


def information(rec, name="information"):
    return np.asarray(rec[name], dtype=np.float64).reshape(6, 6)


def check_record(rec, ref, photometric=True):
    """One device record (a row of odometry.GEOMETRIC_SYSTEM_DTYPE) against blocks(): both row counts exact, then the three
    bar sets.  photometric=False leaves the photometric block and the sum out (a NaN in I1 makes them NaN on both sides).
    Returns the worst ratio to a bar."""
    assert int(rec["rows"]) == ref["rows"], (int(rec["rows"]), ref["rows"])
    assert int(rec["depth_rows"]) == ref["depth_rows"], (int(rec["depth_rows"]), ref["depth_rows"])
    worst = 0.0
    sets = [("depth", information(rec, "depth_information"), rec["depth_gradient"], ref["depth_rows"], rec["depth_cost"],
             ref["H_D"], ref["g_D"], ref["depth_rows"], ref["depth_cost"])]
    if photometric:
        sets += [("photometric", information(rec, "photometric_information"), rec["photometric_gradient"], ref["rows"],
                  rec["photometric_cost"], ref["H_I"], ref["g_I"], ref["rows"], ref["photometric_cost"]),
                 ("sum", information(rec), rec["gradient"], ref["rows"], rec["photometric_cost"] + rec["depth_cost"],
                  ref["H_I"] + ref["H_D"], ref["g_I"] + ref["g_D"], ref["rows"], ref["photometric_cost"] + ref["depth_cost"])]
    for name, h, g, rows, cost, rh, rg, rrows, rcost in sets:
        if rrows == 0:                                     # an empty block: all-zero bits on both sides
            assert not np.any(rh) and not np.any(rg) and rcost == 0.0
            assert not np.any(np.asarray(h).view(np.uint64)) and not np.any(np.asarray(g, dtype=np.float64).view(np.uint64))
            assert np.float64(cost).view(np.uint64) == 0
            continue
        dh, dg = ssr.check_against(h, np.asarray(g, dtype=np.float64), rows, float(cost), rh, rg, rrows, rcost)
        dc = abs(float(cost) - rcost) / (1e-12 * abs(rcost)) if rcost != 0 else 0.0
        print(f"  {name}: |dH| / bar {dh / 1e-10:.3e}, |dg| / bar {dg:.3e}, |dcost| / bar {dc:.3e}")
        worst = max(worst, dh / 1e-10, dg, dc)
    return worst


def parse_line(line):
    """A line of phovo_geometric_system_format -> dict(timestamp, rows, depth_rows, photometric_cost, depth_cost,
    photometric_information[6,6], depth_information[6,6], information[6,6]); the sum with the one add per entry that the
    record's own `information` was built with."""
    f = line.split()
    assert len(f) == 5 + 42, len(f)
    out = dict(timestamp=float(f[0]), rows=int(f[1]), depth_rows=int(f[2]), photometric_cost=float(f[3]), depth_cost=float(f[4]))
    iu = np.triu_indices(6)
    for name, at in (("photometric_information", 5), ("depth_information", 26)):
        h = np.zeros((6, 6))
        h[iu] = [float(x) for x in f[at:at + 21]]
        out[name] = h + np.triu(h, 1).T
    out["information"] = out["photometric_information"] + out["depth_information"]
    return out
