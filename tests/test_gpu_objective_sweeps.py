"""The bi-objective, trust-region and evaluate kernels against their checkers, on the MI355X (-m gpu):

* exact positions: inputs on which every operation of the warp is exact (focal length 64, integer principal point, depth
  1, zero rotation), so that each kernel's rounding or tap rule decides every pixel at once -- C round() at exact halves
  for the bi-objective and evaluate kernels (synthetic.half_pixel_problem, both signs), LinearInitAxis's truncation and
  clamp for the trust region (u, v at c +- 0.25 and c +- 0.75).  Depth exactly at both bounds of the gate, and for a
  non-default range depths that only the default range would let through, are excluded;
* the randomised sweep tests/tools/fuzz_objectives.py in each mode (longer sweeps: DESIGN.md sections 10-12).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import biobjective_ref as bref
import test_gpu_trust_region as gtr
import trust_region_ref as tref
from test_gpu_large_rotations import _cond
from test_gpu_pair_system import _check_against, _numpy_system, _oracle_trace_system

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "fuzz_objectives.py")
RANGES = [(0.3, 5.0), (0.5, 2.0)]
RANGE_IDS = ["default_range", "range_0.5_2"]
PAIRS = 3


def _exact_problem(w, h, shift, depth_range):
    """half_pixel_problem's planes with translation (shift, shift, 0) / 64, and depth marks that the gate must exclude: a
    column at min_depth and a row at max_depth; for a non-default range also a column at 0.4 and a row at 3.0 (inside
    0.3 / 5.0, outside the range in force)."""
    K, i0, d0, i1, _ = synthetic.half_pixel_problem(w, h)
    lo, hi = depth_range
    d0[:, w // 3] = lo
    d0[h // 3, :] = hi
    if depth_range != (0.3, 5.0):
        d0[:, (2 * w) // 3] = 0.4
        d0[(2 * h) // 3, :] = 3.0
    state = np.array([shift / 64.0, shift / 64.0, 0.0, 0.0, 0.0, 0.0])
    gx, gy = oracle.scharr(i1, 0.0625)
    return K, i0, d0, i1, gx, gy, state


def _expected_rows(d0, shift, rounding):
    """Source pixels of depth 1 whose target is in the image: C round() of c + shift (half away from zero) or, for the
    trust region, the real position c + shift in [0, W)."""
    h, w = d0.shape
    c = np.arange(w) + shift
    r = np.arange(h) + shift
    if rounding:
        c, r = np.sign(c) * np.floor(np.abs(c) + 0.5), np.sign(r) * np.floor(np.abs(r) + 0.5)
    cin, rin = (c >= 0) & (c < w), (r >= 0) & (r < h)
    return int(np.sum((d0 == 1.0) & rin[:, None] & cin[None, :]))


# (size, threads, owner map in LDS): the three geometries of the bi-objective and trust-region kernels
GEOMETRIES = [((80, 60), 256, True), ((200, 150), 512, True), ((320, 240), 512, False)]
GEOMETRY_IDS = ["lds256_80x60", "lds512_200x150", "hbm_320x240"]


@pytest.mark.parametrize("depth_range", RANGES, ids=RANGE_IDS)
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus_half", "minus_half"])
@pytest.mark.parametrize("size,threads,in_lds", GEOMETRIES, ids=GEOMETRY_IDS)
def test_biobjective_exact_half_pixel_positions(size, threads, in_lds, sign, depth_range):
    """Every projected coordinate is an exact half: C round() sends c + 0.5 to c + 1 and c - 0.5 to c, and -0.5 to -1
    (out of the image).  The bi-objective decides with `tc > -0.5 && round_half_up_from(tc) < W`; rounded the other way,
    every residual pairs with the wrong pixel, and a -0.5 let through lands on the previous row.  Target depth all ones;
    the engine recomputes its depth gradients and gain from the planes set."""
    w, h = size
    lo, hi = depth_range
    K, i0, d0, i1, gx, gy, state = _exact_problem(w, h, 0.5 * sign, depth_range)
    ones = np.ones((h, w))
    ncfg = native.make_config(num_levels=1, max_iter=[1], min_grad=[0.0])
    ocfg = oracle.make_config(num_levels=1, max_iter=[1], min_grad=[0.0])
    with odometry.AlignmentEngine(0) as e:
        e.set_config(ncfg)
        e.set_intrinsic_matrix(K)
        e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
        e.set_depth_range(lo, hi)
        e.reserve_frames(2, w, h)
        e.set_level_planes(0, 0, intensity=i0, depth=d0)
        e.set_level_planes(1, 0, intensity=i1, depth=ones, grad_x=gx, grad_y=gy)
        dgx, dgy = e.get_level_depth_gradients(1, 0)
        gain = e.get_level_depth_gain(1, 0)
        s, reps = e.align_pairs([0] * PAIRS, [1] * PAIRS, init_states=np.tile(state, (PAIRS, 1)), want_reports=True)
        launches = e.last_launches()
    assert [(r["kind"], r["threads"]) for r in launches] == [("biobjective", threads)], launches
    assert (launches[0]["lds_bytes"] >= 4 * w * h) == in_lds
    cdgx, cdgy = oracle.scharr(ones * (1.0 / hi), ncfg.image_gradients_scaling_factor[0])
    assert np.array_equal(dgx, cdgx) and np.array_equal(dgy, cdgy)
    assert abs(gain - np.mean(i1)) <= 1e-14 * np.mean(i1)
    tgt = dict(i1=[i1], d1=[ones], gx=[gx], gy=[gy], dgx=[cdgx], dgy=[cdgy], gain=[np.mean(i1) / np.mean(ones)])
    es, its, valid, flags, tr = bref.optimize(ocfg, K, ([i0], [d0]), tgt, state, lo, hi)
    expected = _expected_rows(d0, 0.5 * sign, True)
    assert valid == [expected] and its == [1] and flags == 0 and np.all(np.isfinite(es)), (valid, expected, its, flags)
    bar = min(1e-5, 1e-9 * max(1.0, _cond([dict(hessian=t["H"]) for t in tr]) / 1e5))
    for k in range(PAIRS):
        assert list(reps[k].valid_pixels[:1]) == [expected], (k, reps[k].valid_pixels[0], expected)
        assert list(reps[k].iterations[:1]) == [1] and reps[k].flags == 0, (k, reps[k].flags)
        assert np.array_equal(s[k], s[0])
    assert se3.state_distance(s[0], es) < bar, (se3.state_distance(s[0], es), bar)


@pytest.mark.parametrize("depth_range", RANGES, ids=RANGE_IDS)
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus_half", "minus_half"])
@pytest.mark.parametrize("w,h,tiles", [(24, 20, 1), (80, 60, 5), (320, 240, 75)], ids=["tile1", "tiles5", "tiles75"])
def test_evaluate_exact_half_pixel_positions(w, h, tiles, sign, depth_range):
    """The evaluate kernels (fast_rcp, then C round() and the bounds of the analytic objective) at exact halves, one tile
    to many: rows, J^T J, J^T r and cost against the oracle on the same planes, under the depth range in force."""
    assert -(-(-(-(w * h) // 64)) // 16) == tiles             # (the tile count the level size implies: 16 chunks per tile)
    lo, hi = depth_range
    K, i0, d0, i1, gx, gy, state = _exact_problem(w, h, 0.5 * sign, depth_range)
    with odometry.AlignmentEngine(0) as e:
        e.set_config(native.make_config(num_levels=1, max_iter=[1], min_grad=[0.0]))
        e.set_intrinsic_matrix(K)
        e.reserve_frames(2, w, h)
        e.set_level_planes(0, 0, intensity=i0, depth=d0)
        e.set_level_planes(1, 0, intensity=i1, grad_x=gx, grad_y=gy)
        e.set_depth_range(lo, hi)
        out = e.evaluate_pairs([0] * PAIRS, [1] * PAIRS, np.tile(state, (PAIRS, 1)), 0)
    planes = [[i0], [d0], [i1], [gx], [gy]]
    rows, H, g = _oracle_trace_system(planes, 0, K, state, None, lo, hi)
    _, _, cost = _numpy_system(planes, 0, K, state, None, lo, hi)
    expected = _expected_rows(d0, 0.5 * sign, True)
    assert rows == expected, (rows, expected)
    for k in range(PAIRS):
        _check_against(out["information"][k], out["gradient"][k], int(out["rows"][k]), float(out["cost"][k]),
                       H, g, rows, cost)
        assert out["flags"][k] == 0


SHIFTS = [(0.25, "low"), (-0.25, None), (0.75, "clamp"), (-0.75, "low")]


@pytest.mark.parametrize("depth_range", RANGES, ids=RANGE_IDS)
@pytest.mark.parametrize("shift,edge", SHIFTS, ids=["plus_quarter", "minus_quarter", "plus_three_quarters",
                                                    "minus_three_quarters"])
@pytest.mark.parametrize("size,threads,in_lds", GEOMETRIES, ids=GEOMETRY_IDS)
def test_trust_region_exact_tap_positions(size, threads, in_lds, shift, edge, depth_range):
    """u = c + shift and v = r + shift exactly (focal length 64, depth 1): LinearInitAxis after the -0.5 shift truncates
    toward zero, so u in [0, 0.5) keeps taps (0, 1) with a tap weight above 1 (1.25 at u = 0.25), and u in [W - 0.5, W)
    clamps both taps to W - 1; along rows alike.  The first evaluation (rows, cost) equals the checker's to 1e-12, then
    three LM steps through test_gpu_trust_region.compare_pair."""
    w, h = size
    lo, hi = depth_range
    K, i0, d0, i1, gx, gy, state = _exact_problem(w, h, shift, depth_range)
    _, opt = gtr._fixture("config_only_level_0_ceres.yml")
    cfg = native.make_config(num_levels=1, max_iter=[3], min_grad=[0.0])
    with gtr._engine(cfg, opt, K) as e:
        e.set_depth_range(lo, hi)
        e.reserve_frames(2, w, h)
        e.set_level_planes(0, 0, intensity=i0, depth=d0)
        e.set_level_planes(1, 0, intensity=i1, grad_x=gx, grad_y=gy)
        s, reps = e.align_pairs([0] * PAIRS, [1] * PAIRS, init_states=np.tile(state, (PAIRS, 1)), want_reports=True)
        tr = e.trust_region_reports(PAIRS)
        launches = e.last_launches()
    assert [(r["kind"], r["threads"]) for r in launches] == [("trust_region", threads)], launches
    assert (launches[0]["lds_bytes"] >= 4 * w * h) == in_lds
    ev = tref.evaluate(i0, d0, i1, gx, gy, 0, K, state, lo, hi)
    ok, u, v = ev["ok"], ev["u"], ev["v"]
    low = int(np.sum(ok & (u < 0.5))) + int(np.sum(ok & (v < 0.5)))
    clamp = int(np.sum(ok & (u >= w - 0.5))) + int(np.sum(ok & (v >= h - 0.5)))
    assert (low > 0) == (edge == "low") and (clamp > 0) == (edge == "clamp"), (low, clamp)
    assert ev["rows"] == _expected_rows(d0, shift, False), (ev["rows"], _expected_rows(d0, shift, False))
    assert abs(tr["initial_cost"][0, 0] - ev["cost"]) <= 1e-12 * ev["cost"], (tr["initial_cost"][0, 0], ev["cost"])
    xs, rec = tref.optimize_level(lambda x: tref.evaluate(i0, d0, i1, gx, gy, 0, K, x, lo, hi), state, 3,
                                  **tref.level_options(opt, 0))
    assert min(rec["margins"], default=1.0) > gtr.MARGIN, rec["decisions"]
    for k in range(PAIRS):
        assert np.array_equal(s[k], s[0]) and tr[k:k + 1].tobytes() == tr[0:1].tobytes(), k
    gtr.compare_pair(0, s[0], reps[0], tr, xs, {0: rec}, 1)


# ---- the randomised sweeps ---------------------------------------------------------------------------------------
SWEEPS = [("bi", 1000, 11, ("lds256", "lds512", "hbm512")),
          ("tr", 1000, 12, ("lds256", "lds512", "hbm512")),
          ("eval", 1000, 13, ("tiles1", "tiles2-16", "tiles17+"))]


@pytest.mark.parametrize("mode,cases,seed,geometries", SWEEPS, ids=[s[0] for s in SWEEPS])
def test_randomised_sweep_against_checker(mode, cases, seed, geometries):
    """tests/tools/fuzz_objectives.py: `cases` random problems of one kernel, 0 failures, every geometry of the kernel
    exercised (for `eval`: every tile class, as predicted from the level sizes), fewer than 5 % of the cases set aside as
    knife-edge."""
    r = subprocess.run([sys.executable, TOOL, str(cases), str(seed), mode], capture_output=True, text=True, timeout=300)
    out = r.stdout
    assert r.returncode == 0, out[-3000:] + r.stderr[-2000:]
    m = re.search(r"^(\d+) cases, (\d+) failures, (\d+) skipped", out, re.M)
    assert m and int(m.group(1)) == cases and int(m.group(2)) == 0, out[-3000:]
    assert int(m.group(3)) < 0.05 * cases, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith("geometries exercised")][0]
    for g in geometries:
        assert re.search(rf"\b{re.escape(g)}: \d+", line), (g, line)


# Trust-region cases of the long sweeps that missed _check's flat bars with every decision, row count and flag alike: a
# 5x45 strip whose final cost moved by 1.4e-9 (seed 102 case 941), multi-level cases whose finer level's Jacobi scaling
# moved with a rounding-level difference of its entering state (1451, 1597, 1827, 2307), strips of one or two pixels
# whose near-singular LM step carries rounding into a pose hundreds of radians away (seed 102 case 1157; `big` seed 202
# cases 436 and 893, rank-deficient with 0-2 rows left).  They pass under the bars conditioned on cond(J^T J)
# (fuzz_objectives.conditioned_allowance); none may be set aside.
# Then the final radius, moved through rho by the same pose difference: a 236x32 level (seed 12 case 302, cond 3.3e6), a
# 1x37 strip left with 2 rows (983), a 2x49 strip left with 1 row (`big` seed 202 case 572).
TR_REPLAYS = [("941,1451,1597,1827,2307,1157", 2400, 102, ()), ("302,983", 1000, 12, ()),
              ("436,572,893", 900, 202, ("big",))]


@pytest.mark.parametrize("only,cases,seed,flags", TR_REPLAYS, ids=["seed102", "seed12", "seed202_big"])
def test_trust_region_sweep_regressions(only, cases, seed, flags):
    env = dict(os.environ, FUZZ_ONLY=only)
    r = subprocess.run([sys.executable, TOOL, str(cases), str(seed), "tr", *flags], capture_output=True, text=True,
                       timeout=300, env=env)
    n = len(only.split(","))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(rf"^{n} cases, 0 failures, 0 skipped", r.stdout, re.M), r.stdout[-3000:]
