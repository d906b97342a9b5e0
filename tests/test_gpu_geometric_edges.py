"""The photometric-geometric kernels (gn_geometric_kernel.hip; gn_evaluate_geometric_kernels.hip, §17) where
tests/test_gpu_geometric.py and tests/test_gpu_geometric_system.py do not reach: rows, clamped taps and tap gates at exact
positions under two depth ranges (A), initial states in every branch of the device's sin / cos and non-finite ones (B), the
persistent loop with a start state per pair (C), degenerate pairs beside healthy ones and a skipped level (D), 5, 6 and 7
photometric rows (E), levels ended by their thresholds at small sizes (F), the evaluate kernel's tile boundaries and the
aligner's chunk counts (G).  References: geometric_ref.optimize for the aligner and geometric_system_ref.blocks for the
evaluate call, in fp64 on the planes the device holds.  Bars: test_gpu_geometric._compare's and
geometric_system_ref.check_record's, imported, none new.  Every fixture lives in tests/geometric_edges.py and is pre-checked
without a device by tests/test_geometric_edges_cpu.py (margins, flatness, closed-form counts, band and branch counters)."""
import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native

import affine_edges as ae
import edge_states
import geometric_cases as gc
import geometric_edges as ge
import geometric_ref as gr
import geometric_system_ref as gsr
# (helpers of the two existing GPU files, used as they are so that all files hold the device to the same bars)
from test_gpu_geometric import MARGIN_FLOOR, _bits, _compare, _device_pyramid, _engine, _report_words
from test_gpu_geometric_system import _options, _photometric_block_is, _planes, _sampled_on_the_same_pool

assert ge.MARGIN_FLOOR == MARGIN_FLOOR == gsr.MARGIN_FLOOR

pytestmark = pytest.mark.gpu

RANK_DEFICIENT, NONFINITE = native.PAIR_RANK_DEFICIENT, native.PAIR_NONFINITE


def _case(pair, K, c, init=ge.START):
    """A checker configuration (geometric_edges.cfg) as a case of tests/geometric_cases.py, for test_gpu_geometric._engine."""
    return gc._case(pair, c["num_levels"], c["max_iter"], mg=c["min_grad"], lam=c["lam"], weight=c["depth_weight"],
                    limit=c["max_depth_residual"], init=init, K=K)


def _open(pair, K, c, frames=2):
    eng = _engine(_case(pair, K, c), frames=frames)
    eng.set_depth_range(c["min_depth"], c["max_depth"])
    return eng


def _blank_pair(w, h):
    """Frames to reserve a pool with; every plane a test reads is then set through set_level_planes."""
    g, d = np.zeros((h, w), dtype=np.uint8), np.ones((h, w))
    return dict(gray0=g, depth0=d, gray1=g, depth1=d)


def _set_planes(eng, planes, level=0):
    """The source's intensity and depth; the target's intensity, Scharr gradients and depth (which gives it the source role)."""
    i0, d0, i1, gx, gy, d1 = planes
    eng.set_level_planes(0, level, intensity=i0, depth=d0)
    eng.set_level_planes(1, level, intensity=i1, depth=d1, grad_x=gx, grad_y=gy)


def _align(eng, src, tgt, inits):
    """One enqueue -> (states, reports, geometric records)."""
    n = len(src)
    s, reps = eng.align_pairs(src, tgt, init_states=np.asarray(inits, dtype=np.float64).reshape(n, 6), want_reports=True)
    g = eng.fetch_geometric_reports(n)
    assert {l["kind"] for l in eng.last_launches()} == {"geometric"}
    return s, reps, g


def _record(s, rep, g, nl):
    """Everything a pair reports, for bit-for-bit comparison: pose, report, geometric record."""
    return _bits(s), _report_words(rep, g, nl)


def _hold(part, what, s, rep, g, ref, nl, expect_flat=True):
    """test_gpu_geometric._compare, and the distance / bar of the pair printed for DESIGN.md §16's table."""
    _compare(s, rep, g, ref, nl, expect_flat=expect_flat)
    if np.all(np.isfinite(ref["state"])):
        ratio = np.abs(s - ref["state"]).max() / gr.pose_bar(ref["cond"], ref["state"])
        print(f"part {part} {what}: distance / bar {ratio:.3e}")


def _hold_system(part, what, rec, ref):
    """geometric_system_ref.check_record with the margins and the flags of test_gpu_geometric_system, and the worst
    distance / bar printed for DESIGN.md §17's table."""
    assert ref["cell_margin"] > gc.CELL_FLOOR and ref["gate_margin"] > gsr.MARGIN_FLOOR, what
    worst = gsr.check_record(rec, ref)
    assert int(rec["flags"]) == (RANK_DEFICIENT if ref["rows"] < 6 else 0), what
    if ref["rows"] == 0:                                       # an empty system: every sum has all-zero bits
        assert rec.tobytes()[:1024] == bytes(1024), what
    print(f"part {part} evaluate {what}: rows {ref['rows']} depth rows {ref['depth_rows']} distance / bar {worst:.3e}")
    return worst


def _three_alike(s, reps, g, nl):
    for k in range(1, len(s)):
        assert _record(s[k], reps[k], g[k], nl) == _record(s[0], reps[0], g[0], nl), k


# ---- A. exact positions ------------------------------------------------------------------------------------------------
EXACT_CASES = [(w, h, s, r) for (w, h), shifts in ge.EXACT_SIZES.items() for s in shifts for r in ge.RANGES]


@pytest.mark.parametrize("w,h,shift,depth_range", EXACT_CASES,
                         ids=[f"{w}x{h}_{s:+.2f}_{r[0]}_{r[1]}" for w, h, s, r in EXACT_CASES])
def test_geometric_exact_rows_and_taps(w, h, shift, depth_range):
    """Every projected coordinate is exactly c + shift, r + shift: at +-0.5 the outermost column and row sit on -0.5 /
    W - 0.5 and are out (both comparisons are strict), at +-0.25 they are rows whose taps are clamped and whose depth
    derivative across the clamp is exactly 0, at +-0.75 they are out.  Source pixels and target taps AT min_depth and AT
    max_depth are out, a NaN tap is out, and under 0.5 / 2.0 so are depths 0.4 and 3.0, which 0.3 / 5.0 lets through.  The
    target depth lies on the 1/64 grid, so the D1 sample and the residual at the gate are exact.  Aligner (one iteration,
    three copies, bit-identical) and evaluate call, on the same planes; both once more with the residual gate off, where
    a tap at max_depth that slipped through the tap gate cannot hide behind its large residual."""
    K, planes, state = ge.exact_problem(w, h, shift, depth_range)
    expected = ae.exact_rows(planes[1], shift)
    c = ge.exact_cfg(depth_range)
    with _open(_blank_pair(w, h), K, c) as eng:
        _set_planes(eng, planes)
        s, reps, g = _align(eng, [0] * 3, [1] * 3, np.tile(state, (3, 1)))
        rec = eng.evaluate_geometric_pairs([0], [1], state[None], 0)[0]
        sampled = _sampled_on_the_same_pool(eng, [0], [1], state[None], 0)[0]
        _options(eng, ge.EXACT_SIGMA, 0.0)                     # the residual gate off: every tap the tap gate passes is a depth row
        s_off, reps_off, g_off = _align(eng, [0], [1], state)
        rec_off = eng.evaluate_geometric_pairs([0], [1], state[None], 0)[0]
    ref = gr.optimize([planes], K, c, state)
    assert ref["valid_pixels"] == [expected] and ref["iterations"] == [1] and ref["flags"] == 0
    assert list(reps[0].valid_pixels[:1]) == [expected]
    _three_alike(s, reps, g, 1)
    _hold("A", f"{w}x{h} {shift:+.2f} {depth_range}", s[0], reps[0], g[0], ref, 1)
    blocks = gsr.blocks(planes, 0, K, state, ge.EXACT_SIGMA, ge.EXACT_LIMIT, *depth_range)
    assert (blocks["rows"], blocks["depth_rows"]) == (expected, ref["depth_rows"][0])
    _hold_system("A", f"{w}x{h} {shift:+.2f} {depth_range}", rec, blocks)
    _photometric_block_is(rec, sampled)
    ref_off = gr.optimize([planes], K, dict(c, max_depth_residual=[0.0]), state)
    assert ref_off["depth_rows"][0] > ref["depth_rows"][0]
    _hold("A", f"{w}x{h} {shift:+.2f} {depth_range} gate off", s_off[0], reps_off[0], g_off[0], ref_off, 1)
    _hold_system("A", f"{w}x{h} {shift:+.2f} {depth_range} gate off", rec_off,
                 gsr.blocks(planes, 0, K, state, ge.EXACT_SIGMA, 0.0, *depth_range))
    _photometric_block_is(rec_off, sampled)


# ---- B. large angles ---------------------------------------------------------------------------------------------------
def test_geometric_initial_states_in_every_branch():
    """edge_states.initial_states() (branches 2 and 3 of write_pose_constants on each axis, both signs, pi - 0.3 on pitch
    and roll) as one batch, three fixed iterations on each of two levels, sigma 2, gate off: Cm = dZ'/dpitch and Dm =
    dZ'/droll with t16, t17 and t24 far from their small-angle values.  Rows, depth rows, flags and the iteration at which a
    state stops being finite equal the checker's; the pose is within pose_bar, the flat one for every finite state."""
    p = ge.angle_pair()
    c = ge.angle_cfg()
    inits = np.array(edge_states.initial_states())
    n, nl = len(inits), 2
    with _open(p, p["K"], c) as eng:
        pyr = _device_pyramid(eng, 0, 1, nl, ge.ANGLE_MAX_ITER)
        s, reps, g = _align(eng, [0] * n, [1] * n, inits)
    classes, good = dict(flat=0, conditioned=0, nonfinite=0), set()
    for i in range(n):
        ref = gr.optimize(pyr, p["K"], c, inits[i])
        kind = ge.angle_class(ref)
        classes[kind] += 1
        if kind == "flat" and min(ref["valid_pixels"]) > 100:
            good.add(ae.angle_label(inits[i]))
        _hold("B", f"state {i} {ae.angle_label(inits[i])}", s[i], reps[i], g[i], ref, nl, expect_flat=kind == "flat")
    # on the planes the device holds, as on the CPU pyramid (test_geometric_edges_cpu.py): every axis, sign and branch keeps
    # a pair under the flat bar with more than 100 rows on both levels
    assert good == ge.ALL_LABELS, ge.ALL_LABELS - good
    assert classes == ge.ANGLE_CLASSES, classes


def test_geometric_system_at_every_branch():
    """The evaluate call at the same 32 states, on both levels, gate off and on; a state that sees no row gives the all-zero
    record with RANK_DEFICIENT."""
    p = ge.angle_pair()
    inits = np.array(edge_states.initial_states())
    n = len(inits)
    worst, empty = 0.0, 0
    with _open(p, p["K"], ge.angle_cfg()) as eng:
        for level in (0, 1):
            planes = _planes(eng, level)
            for limit in ge.ANGLE_EVAL_LIMITS:
                _options(eng, ge.ANGLE_SIGMA, limit)
                recs = eng.evaluate_geometric_pairs([0] * n, [1] * n, inits, level)
                for i in range(n):
                    ref = gsr.blocks(planes, level, p["K"], inits[i], ge.ANGLE_SIGMA, limit)
                    worst = max(worst, _hold_system("B", f"state {i} level {level} limit {limit}", recs[i], ref))
                    empty += ref["rows"] == 0
    assert empty == 16
    print(f"part B evaluate: worst distance / bar {worst:.3e}")


def test_geometric_large_in_plane_motions():
    """True yaw of 0.5, 0.7 and 0.9 rad (branches 2, 2, 3), started near the truth, gate 0.1 m, ended by the gradient
    threshold (the depth rows are in the g it tests)."""
    c = ge.motion_cfg()
    for p, init in ae.motion_pairs():
        with _open(p, p["K"], c) as eng:
            pyr = _device_pyramid(eng, 0, 1, 1, ge.MOTION_MAX_ITER)
            s, reps, g = _align(eng, [0] * 3, [1] * 3, np.tile(init, (3, 1)))
        ref = gr.optimize(pyr, p["K"], c, init)
        assert ref["iterations"][0] < ge.MOTION_MAX_ITER[0] and abs(ref["state"][3] - p["motion"][3]) < 0.05
        _hold("B", f"yaw {p['motion'][3]}", s[0], reps[0], g[0], ref, 1)
        _three_alike(s, reps, g, 1)


def test_geometric_nonfinite_initial_angle():
    """A NaN and an inf initial yaw among eight healthy pairs: the healthy ones keep the bits of the batch without them,
    the two report what the checker does (no row, NONFINITE and RANK_DEFICIENT after one iteration on every level, a
    geometric record of zeros)."""
    p = ge.angle_pair()
    c = ge.angle_cfg()
    states, bad = ae.nonfinite_batch()
    good = [k for k in range(len(states)) if k not in bad]
    nl = 2
    with _open(p, p["K"], c) as eng:
        pyr = _device_pyramid(eng, 0, 1, nl, ge.ANGLE_MAX_ITER)
        s, reps, g = _align(eng, [0] * len(states), [1] * len(states), states)
        s2, reps2, g2 = _align(eng, [0] * len(good), [1] * len(good), states[good])
    for j, k in enumerate(good):
        assert _record(s[k], reps[k], g[k], nl) == _record(s2[j], reps2[j], g2[j], nl), k
        assert reps[k].flags == 0
    _hold("B", "healthy beside NaN / inf", s[0], reps[0], g[0], gr.optimize(pyr, p["K"], c, states[0]), nl)
    for k in bad:
        ref = gr.optimize(pyr, p["K"], c, states[k])
        assert ref["iterations"] == [1, 1] and ref["flags"] == gr.PAIR_RANK_DEFICIENT | gr.PAIR_NONFINITE
        _hold("B", f"bad yaw {states[k][3]}", s[k], reps[k], g[k], ref, nl)
        assert list(g[k]["depth_rows"][:nl]) == [0, 0] and _bits(g[k]["photometric_cost"][:nl]) == [0, 0]
        assert _bits(g[k]["depth_cost"][:nl]) == [0, 0]


# ---- C. the work queue with per-pair start states ------------------------------------------------------------------------
def test_geometric_work_queue_reads_every_pairs_own_start_state():
    """520 positions drawn from the four 24x20 pair kinds of test_work_queue_hands_every_pair_its_own_bits (healthy, no depth
    row, no row, another healthy pair), each from one of six non-zero start states: more pairs than workgroups, so
    A.states[pair] is read on a second trip through the persistent loop.  Every (pair, state) combination aligned alone is
    held to the checker; then every position has its combination's bits -- pose, report and geometric record."""
    K, frames = ge.work_queue_frames()
    c = ge.work_queue_cfg()
    nl = ge.WQ_LEVELS
    states, pick, which = ge.work_queue_draw()
    kinds = np.array(ge.WQ_KINDS)
    with _open(dict(gray0=frames[0][0], depth0=frames[0][1], gray1=frames[1][0], depth1=frames[1][1]), K, c, frames=6) as eng:
        for f in range(2, 6):
            eng.upload_frame(f, *frames[f])
        pyr = [_device_pyramid(eng, a, b, nl, ge.WQ_MAX_ITER) for a, b in ge.WQ_KINDS]
        combos = sorted({(int(a), int(b)) for a, b in zip(which, pick)})
        alone = {}
        for a, b in combos:
            s, reps, g = _align(eng, [kinds[a][0]], [kinds[a][1]], states[b])
            assert eng.last_launches()[0]["workgroups"] == 1
            ref = gr.optimize(pyr[a], K, c, states[b])
            _hold("C", f"pair {a} from state {b}", s[0], reps[0], g[0], ref, nl)
            alone[(a, b)] = _record(s[0], reps[0], g[0], nl)
        s, reps, g = _align(eng, kinds[which, 0], kinds[which, 1], states[pick])
        grid = max(l["workgroups"] for l in eng.last_launches())
    assert len(combos) == 24 and ge.WQ_N > grid, (ge.WQ_N, grid)              # fewer workgroups than pairs
    for k in range(ge.WQ_N):
        assert _record(s[k], reps[k], g[k], nl) == alone[(int(which[k]), int(pick[k]))], (k, which[k], pick[k])
    assert len({repr(v) for (a, b), v in alone.items() if a != 2}) == 18         # the start state shows in every healthy record


# ---- D. mixed batch, skipped level -------------------------------------------------------------------------------------
def test_geometric_mixed_batch():
    """Healthy pairs, a target whose depth is invalid everywhere (no depth row), an all-NaN source depth (no row) and a target
    with NaN / 0 / beyond-max holes, in one enqueue of 12 on three levels: every report equals the checker's, the healthy
    pairs keep the bits they have alone."""
    pairs = ge.mixed_pairs()
    kinds = list(ge.MIX_SEEDS)
    nl = ge.MIX_LEVELS
    c = ge.mixed_cfg()
    which = [kinds.index(k) for k in ge.MIX_KINDS]
    src, tgt = [2 * i for i in which], [2 * i + 1 for i in which]
    with _open(pairs[kinds[0]], pairs[kinds[0]]["K"], c, frames=2 * len(kinds)) as eng:
        for i, k in enumerate(kinds):
            eng.upload_frame(2 * i, pairs[k]["gray0"], pairs[k]["depth0"])
            eng.upload_frame(2 * i + 1, pairs[k]["gray1"], pairs[k]["depth1"])
        pyr = [_device_pyramid(eng, 2 * i, 2 * i + 1, nl, ge.MIX_MAX_ITER) for i in range(len(kinds))]
        s, reps, g = _align(eng, src, tgt, np.tile(ge.START, (len(which), 1)))
        alone = {i: _align(eng, [2 * i], [2 * i + 1], ge.START) for i in set(which) if kinds[i].startswith("healthy")}
    assert len(which) == 12 and len(alone) == 3
    refs = [gr.optimize(pyr[i], pairs[k]["K"], c, ge.START) for i, k in enumerate(kinds)]
    for k, i in enumerate(which):
        _hold("D", f"position {k} {kinds[i]}", s[k], reps[k], g[k], refs[i], nl)
        if i in alone:
            a = alone[i]
            assert _record(s[k], reps[k], g[k], nl) == _record(a[0][0], a[1][0], a[2][0], nl), (k, kinds[i])
            assert reps[k].flags == 0
    assert refs[kinds.index("nan_source")]["flags"] == gr.PAIR_RANK_DEFICIENT | gr.PAIR_NONFINITE
    assert refs[kinds.index("no_target_depth")]["depth_rows"] == [0, 0, 0]
    assert refs[kinds.index("target_holes")]["depth_rows"][0] < 0.6 * refs[kinds.index("healthy0")]["depth_rows"][0]


def test_geometric_skipped_level():
    """max_num_iterations [5, 0, 5]: no launch names level 1, it reports one iteration, and its valid_pixels, depth_rows,
    photometric_cost and depth_cost are what the engine defines for a level that did not run -- 0, 0, +0.0, +0.0: both
    records are zeroed before the first level and no kernel writes that level's slots.  The state level 2
    leaves enters level 0, and the result is not that of [5, 5, 5]."""
    p = ge.skip_pair()
    nl = 3
    got = {}
    for mi in (ge.SKIP_MAX_ITER, ge.FULL_MAX_ITER):
        c = ge.skip_cfg(mi)
        with _open(p, p["K"], c) as eng:
            pyr = _device_pyramid(eng, 0, 1, nl, mi)
            s, reps, g = _align(eng, [0], [1], ge.START)
            levels = [l["levels"] for l in eng.last_launches()]
        ref = gr.optimize(pyr, p["K"], c, ge.START)
        assert levels == [[l] for l in (2, 1, 0) if mi[l] > 0], levels
        _hold("D", f"max_iter {mi}", s[0], reps[0], g[0], ref, nl)
        got[tuple(mi)] = (_bits(s[0]), list(reps[0].iterations[:nl]), reps[0], g[0])
    skip, full = got[tuple(ge.SKIP_MAX_ITER)], got[tuple(ge.FULL_MAX_ITER)]
    assert skip[1] == [5, 1, 5] and full[1] == [5, 5, 5]
    assert int(skip[2].valid_pixels[1]) == 0 and int(skip[3]["depth_rows"][1]) == 0
    assert _bits([skip[3]["photometric_cost"][1], skip[3]["depth_cost"][1]]) == [0, 0]
    assert int(full[3]["depth_rows"][1]) > 1000 and full[3]["depth_cost"][1] > 0.0
    assert skip[0] != full[0]


# ---- E. row counts around the rank test ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ge.ROWS_LAYOUTS)
def test_geometric_five_six_and_seven_rows(layout):
    """RANK_DEFICIENT is `fewer than 6 PHOTOMETRIC rows`.  6 and 7 rows of real data with as many depth rows, well posed
    (cond(H) about 5e2): flags 0 and the state within the flat bar after one iteration and after three.  5 + 5 rows: the
    flag is set, and since the depth rows supply the rank (the checker's cond(H) is 5e2 ... 1.2e3 on both seeds) the state
    is held to the flat bar as well.  7 rows under a target depth that fails every tap: 7 rows, 0 depth rows, a depth cost
    of +0.0, the checker's pose.  The rows sit in one chunk of one wave, or in all four waves."""
    seed = ge.ROWS_SEED[layout]
    runs = [(count, mi, True) for count in ge.ROWS_COUNTS for mi in ([1], [ge.ROWS_ITER])]
    runs += [(7, [1], False), (7, [ge.ROWS_ITER], False)]
    for count, mi, target_depth in runs:
        K, planes = ge.rows_problem(seed, layout, count, target_depth)
        c = ge.rows_cfg(mi)
        with _open(_blank_pair(ge.ROWS_W, ge.ROWS_H), K, c) as eng:
            _set_planes(eng, planes)
            s, reps, g = _align(eng, [0] * 3, [1] * 3, np.tile(ge.START, (3, 1)))
        _three_alike(s, reps, g, 1)
        ref = gr.optimize([planes], K, c, ge.START)
        assert ref["valid_pixels"] == [count] and ref["depth_rows"] == [count if target_depth else 0]
        assert ref["flags"] == (gr.PAIR_RANK_DEFICIENT if count < 6 else 0) == int(reps[0].flags)
        _hold("E", f"{layout} {count} rows {'' if target_depth else 'no target depth '}{mi[0]} iterations", s[0], reps[0],
              g[0], ref, 1)
        if not target_depth:
            assert _bits(g[0]["depth_cost"][:1]) == [0] and int(g[0]["depth_rows"][0]) == 0


# ---- F. thresholds at small sizes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ge.THR_SIZES, ids=["24x20", "75x53"])
def test_geometric_thresholds_end_small_levels(w, h):
    """Two levels, lambda [0.7, 0.5], weights [2, 3], gates on, and both levels ended by ||g|| < min_gradient_norm after 4
    to 8 iterations (7 + 5 at 24x20, 8 + 4 at 75x53) -- tested after the step, with the depth rows in g."""
    p = ge.threshold_pair(w, h)
    c = ge.threshold_cfg(w, h)
    with _open(p, p["K"], c) as eng:
        pyr = _device_pyramid(eng, 0, 1, 2, ge.THR_MAX_ITER)
        s, reps, g = _align(eng, [0] * 3, [1] * 3, np.tile(ge.START, (3, 1)))
    ref = gr.optimize(pyr, p["K"], c, ge.START)
    assert all(3 <= it <= 8 for it in ref["iterations"]) and ref["flags"] == 0
    _hold("F", f"{w}x{h}", s[0], reps[0], g[0], ref, 2)
    _three_alike(s, reps, g, 2)


# ---- G. tiles and chunks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ge.TILE_SIZES, ids=[f"{w}x{h}" for w, h in ge.TILE_SIZES])
def test_geometric_system_at_the_tile_boundaries(w, h):
    """1024 pixels (one full tile), 1025 (a second tile of one pixel, which has a depth row at START), 8192 (8 tiles, one per
    subset of the finish kernel) and 8256 (9: subset 0 adds tiles 0 and 8), at START and at a yaw of 0.8 rad, gate off and
    on; the photometric block is the sampled record bit for bit."""
    p = ge.tile_pair(w, h)
    states = ge.tile_states()
    c = ge.cfg([1], weight=ge.TILE_SIGMA)
    with _open(p, p["K"], c) as eng:
        planes = _planes(eng, 0)
        sampled = _sampled_on_the_same_pool(eng, [0, 0], [1, 1], states, 0)
        for limit in ge.TILE_LIMITS:
            _options(eng, ge.TILE_SIGMA, limit)
            recs = eng.evaluate_geometric_pairs([0, 0], [1, 1], states, 0)
            for i in range(2):
                ref = gsr.blocks(planes, 0, p["K"], states[i], ge.TILE_SIGMA, limit)
                assert ref["rows"] > 500 and ref["depth_rows"] > 300
                _hold_system("G", f"{w}x{h} yaw {states[i][3]} limit {limit}", recs[i], ref)
                _photometric_block_is(recs[i], sampled[i])
    tail = gr.rows_vectorised(planes, 0, p["K"], ge.START, ge.TILE_SIGMA, 0.0)["drows"][(w * h - 1) // 1024 * 1024:]
    assert tail.sum() > 0                                      # the last tile holds depth rows on the device's planes too


@pytest.mark.parametrize("w,h", ge.CHUNK_SIZES, ids=[f"{w}x{h}" for w, h in ge.CHUNK_SIZES])
def test_geometric_chunk_counts(w, h):
    """3 chunks (fewer than waves: wave 0 takes one and leaves the loop at its first exit, wave 3 none) and 12 (three per
    wave: the second exit after an odd count); 24x20 elsewhere has two per wave."""
    p = ge.tile_pair(w, h)
    c = ge.cfg(ge.CHUNK_MAX_ITER, weight=ge.CHUNK_SIGMA, limit=ge.CHUNK_LIMIT)
    with _open(p, p["K"], c) as eng:
        pyr = _device_pyramid(eng, 0, 1, 1, ge.CHUNK_MAX_ITER)
        s, reps, g = _align(eng, [0] * 3, [1] * 3, np.tile(ge.START, (3, 1)))
    ref = gr.optimize(pyr, p["K"], c, ge.START)
    assert ref["flags"] == 0 and ref["depth_rows"][0] > 100
    _hold("G", f"{w}x{h} aligner", s[0], reps[0], g[0], ref, 1)
    _three_alike(s, reps, g, 1)
