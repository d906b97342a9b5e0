"""The many-workgroup form of a Gauss-Newton level (csrc/gn_wide_kernels.hip, its call in engine.cpp) at its tile, stop and
batch edges (run with -m gpu on an MI355X).

The inputs are those of tests/wide_form.py; tests/test_wide_form_cpu.py vouches for every one of them without a GPU (tile
counts, what the last tile carries, the stop counts of every batch against the host's look schedule, decision margins of
1e-6, one ulp of fx).  Every case runs under set_wide_policy(1) on fp64 planes with nearest / scatter sampling and asserts
that every launch of the enqueue is "wide".

Bars, the project's own: pose se3.state_distance below the conditioned bar of test_gpu_large_rotations.Expect (1e-9
wherever cond(J^T J) <= 1e5, which the CPU file asserts for the tile cases), iteration counts and valid pixels exact,
gradient norm within 1e-9 relative, flags exact.  Where two runs differ only in who else is in the batch, in the order or
in what the engine did before, the bits are the same: this form's sum order depends on the level size alone.

1. tile counts 1, 2, 7, 8, 9, 16, 17 with last tiles of 1024, 1023, 8 and 1 pixels (the 1- and 8-pixel tiles end in the image's
   corner, whose Scharr gradient is exactly 0 under reflect-101: their check is the exact valid-pixel count);
2. pairs that stop after every iteration count 1 ... 16 in one batch, under limits that make the host look twice, once or
   never and leave at its first or second look; two levels, level 0 entered from either slot of the state buffer;
3. every pair of the mixed batch alone, in the reversed batch, and the same with 40 pairs;
4. a pair without rows among healthy ones, and sources with 3, 4, 5, 6 and 40 valid depths spread over the tiles;
5. projections that are exact halves, through this form's own round();
6. strips one to five pixels wide.
Each case prints its largest pose distance over the bar before it asserts (DESIGN.md section 4 tables them).
"""
import numpy as np
import pytest

import extension_forms as ef
import wide_form as wf

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3

pytestmark = pytest.mark.gpu

GRAD_TOL = wf.GRAD_TOL


# ------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------
def _engine(ncfg, K, size, n_frames=2):
    e = odometry.AlignmentEngine()
    e.set_config(ncfg)
    e.set_intrinsic_matrix(K)
    e.set_depth_range(wf.MIN_DEPTH, wf.MAX_DEPTH)
    e.set_wide_policy(1)
    e.reserve_frames(n_frames, size[0], size[1])
    return e


def _upload(e, p, src=0, tgt=1):
    e.upload_frame(src, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
    e.upload_frame(tgt, p["gray1"], None, roles=native.ROLE_TARGET)


def _align(e, src, tgt, inits=None, levels=1):
    """One enqueue; every launch of it is of this form, one per level, coarse to fine."""
    out = e.align_pairs(src, tgt, init_states=None if inits is None else np.asarray(inits, dtype=np.float64),
                        want_reports=True)
    launches = e.last_launches()
    assert [r["kind"] for r in launches] == ["wide"] * levels, launches
    assert all(r["threads"] == 256 for r in launches), launches
    return out


def _report_tuple(r, nl):
    return (list(r.iterations[:nl]), list(r.valid_pixels[:nl]), r.gradient_norm, r.flags)


def _same_bits(a, b, what, nl=1, pairs_a=None, pairs_b=None):
    """States and reports of two runs bit for bit: pair pairs_a[k] of a against pair pairs_b[k] of b."""
    (sa, ra), (sb, rb) = a, b
    pairs_a = range(len(sa)) if pairs_a is None else pairs_a
    pairs_b = range(len(sb)) if pairs_b is None else pairs_b
    assert len(pairs_a) == len(pairs_b)
    for i, j in zip(pairs_a, pairs_b):
        assert sa[i].tobytes() == sb[j].tobytes(), (what, i, j, sa[i], sb[j])
        ta, tb = _report_tuple(ra[i], nl), _report_tuple(rb[j], nl)
        assert ta[:2] == tb[:2] and ta[3] == tb[3], (what, i, j, ta, tb)
        assert ta[2] == tb[2] or (np.isnan(ta[2]) and np.isnan(tb[2])), (what, i, j, ta, tb)


def _check(ref, state, rep, what):
    """One pair against its reference; returns distance / bar."""
    nl = ref.nl
    assert list(rep.iterations[:nl]) == ref.its, (what, list(rep.iterations[:nl]), ref.its)
    assert list(rep.valid_pixels[:nl]) == ref.valid, (what, list(rep.valid_pixels[:nl]), ref.valid)
    assert rep.flags == ref.flags, (what, rep.flags, ref.flags)
    assert abs(rep.gradient_norm - ref.gnorm) <= GRAD_TOL * max(1.0, ref.gnorm), (what, rep.gradient_norm, ref.gnorm)
    d = se3.state_distance(state, ref.state)
    assert d < ref.bar, (what, d, ref.bar)
    return d / ref.bar


def _check_all(refs, got, what):
    states, reps = got
    assert len(states) == len(refs)
    worst = max(_check(r, states[k], reps[k], (what, k)) for k, r in enumerate(refs))
    print(f"wide form {what}: {len(refs)} pairs, iterations {sorted({tuple(r.its) for r in refs})}, "
          f"worst pose distance / bar {worst:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# 1. tile counts and partial tiles
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(wf.TILE_SIZES), ids=wf.size_id)
def test_tile_counts_and_partial_tiles(size):
    """Three pairs, three fixed iterations from the zero state on one level of ceil(n / 1024) tiles.  A tile sum that the
    interleaved loop t = sub, sub + 8, ... forgets, or a lane of the partial last chunk that is dropped, changes the valid
    pixels of the last iteration (tests/test_wide_form_cpu.py: every pixel of the last tile has valid depth and losing the tile
    loses pixels) and, where the tile holds a chunk or more, the pose by more than 1e-6.  The 1- and 8-pixel tiles of 41x25,
    145x113 and 82x100 end in the image's corner, whose Scharr gradient is exactly 0 under reflect-101: the exact
    valid-pixel count is their check.  A second enqueue gives the same bits."""
    pairs = wf.tile_pairs(size)
    refs = [wf.tile_ref(size, i) for i in range(len(pairs))]
    ncfg, _ = wf.cfgs([wf.TILE_ITERS])
    src, tgt = [0, 2, 4], [1, 3, 5]
    with _engine(ncfg, pairs[0]["K"], size, 6) as e:
        for i, p in enumerate(pairs):
            _upload(e, p, 2 * i, 2 * i + 1)
        got = _align(e, src, tgt)
        again = _align(e, src, tgt)
        assert e.last_launches()[0]["workgroups"] == 3 * wf.TILE_SIZES[size][0]
    _check_all(refs, got, f"tiles {wf.size_id(size)} ({wf.TILE_SIZES[size][0]} tiles, {wf.TILE_SIZES[size][1]} px in the last)")
    _same_bits(got, again, size)


# ------------------------------------------------------------------------------------------------------------------------
# 2. stop iteration, buffer parity, host looks
# ------------------------------------------------------------------------------------------------------------------------
def _stop_engine(max_iter, min_grad, size=wf.STOP_SIZE):
    ncfg, _ = wf.cfgs(list(max_iter), list(min_grad))
    p = wf.stop_pair(size)
    e = _engine(ncfg, p["K"], size)
    _upload(e, p)
    return e


def _run_states(e, states, levels=1):
    n = len(states)
    return _align(e, [0] * n, [1] * n, np.array(states), levels)


@pytest.mark.parametrize("name", wf.STOP_BATCHES)
def test_stop_iteration_buffer_parity_and_host_looks(name):
    """One 82x100 pair from searched initial states, gradient threshold 230: every pair of the batch has the oracle's
    iteration count, valid pixels, gradient norm, flags and pose, whichever slot of the state buffer its last step went to
    and whatever the host loop saw.  mixed16: every stop count 1 ... 16, looks after 4 and 12 iterations; mixed13: an odd
    limit; never_looks7 / one_look8: the limits around the first look; leaves_first_look / leaves_second_look: max_iter 50
    with every pair done by iteration 3 / 11, so that the loop ends at a look; no_threshold5: nobody looks.  After a batch
    the loop left early, another pair set on the same engine gives the bits it gives on a fresh engine: the workspace and
    the owner map were left clean."""
    max_iter, thr, states = wf.stop_batches()[name]
    refs = wf.batch_refs(name)
    other = wf.mixed_states()[:8]
    with _stop_engine((max_iter,), (thr,)) as e:
        got = _run_states(e, states)
        behind = _run_states(e, other) if name in wf.EARLY_LEAVING else None
    stops = [r.its[0] for r in refs]
    print(f"wide form {name}: stop counts {sorted(set(stops))}, host looks {wf.host_looks(max_iter, thr)}, "
          f"iterations launched {wf.launched_iterations(max_iter, thr, stops)}")
    _check_all(refs, got, name)
    if behind is not None:
        with _stop_engine((max_iter,), (thr,)) as e:
            fresh = _run_states(e, other)
        _same_bits(behind, fresh, name + ", the next pair set")
        _check_all([wf.stop_ref(s, (max_iter,), (thr,)) for s in other], behind, name + ", the next pair set")


def test_two_levels_enter_level_zero_from_either_slot():
    """164x200, both levels in this form (9 and 33 tiles, 32 pixels in the last): four pairs leave level 1 after an odd count,
    four after an even one, so that k_wide_finish hands the state of either slot to level 0; per-level iterations, valid
    pixels, gradient norm, flags and pose are the oracle's."""
    refs = wf.two_level_refs()
    with _stop_engine(wf.TWO_MAX_ITER, wf.TWO_MIN_GRAD, wf.TWO_SIZE) as e:
        got = _run_states(e, wf.two_level_states(), levels=2)
        again = _run_states(e, wf.two_level_states(), levels=2)
    _check_all(refs, got, "two levels")
    _same_bits(got, again, "two levels", nl=2)


# ------------------------------------------------------------------------------------------------------------------------
# 3. position and batch size
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", wf.POSITION_SIZES)
def test_position_and_batch_size_change_no_bit(n):
    """The mixed batch (32 pairs, and 40: policy 1 takes any count): every pair alone and in the reversed batch gives
    exactly the bits and the report it has in the batch.  The sum order depends on the level size only, so bit equality
    is what must hold."""
    states = wf.mixed_states(n)
    refs = [wf.stop_ref(s, (16,), (wf.THRESHOLD,)) for s in states]
    with _stop_engine((16,), (wf.THRESHOLD,)) as e:
        assert e.level_uses_wide(0, n)
        batch = _run_states(e, states)
        reverse = _run_states(e, states[::-1])
        alone = [_run_states(e, [s]) for s in states]
    _check_all(refs, batch, f"position, {n} pairs")
    _same_bits(batch, reverse, f"reversed, {n} pairs", pairs_a=range(n), pairs_b=range(n - 1, -1, -1))
    for k in range(n):
        _same_bits(batch, alone[k], f"alone, {n} pairs", pairs_a=[k], pairs_b=[0])


# ------------------------------------------------------------------------------------------------------------------------
# 4. no rows and too few rows
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wf.NO_ROWS))
def test_pair_without_valid_pixels_is_flagged_in_the_oracles_iteration(name):
    """test_gpu_serial_section.py's case on this form: one slot of eight starts ten kilometres to the side.  It is flagged
    PAIR_NONFINITE, its iteration counts are the oracle's first non-finite iteration of every executed level, its valid
    pixels 0; its neighbours have the bits of the batch without it and no flag."""
    size, max_iter = wf.NO_ROWS[name]
    nl = len(max_iter)
    bad = wf.no_rows_ref(name, wf.BAD_SLOT)
    assert not bad.finite and bad.first_nonfinite == [1] * nl
    init = np.array(wf.no_rows_states())
    with _stop_engine(max_iter, (0.0,) * nl, size) as e:
        clean = _run_states(e, init, levels=nl)
        init[wf.BAD_SLOT] = wf.NOWHERE
        s, reps = _run_states(e, init, levels=nl)
    r = reps[wf.BAD_SLOT]
    assert r.flags & native.PAIR_NONFINITE and not np.all(np.isfinite(s[wf.BAD_SLOT])), (name, r.flags, s[wf.BAD_SLOT])
    assert list(r.iterations[:nl]) == bad.first_nonfinite, (name, list(r.iterations[:nl]), bad.first_nonfinite)
    assert list(r.valid_pixels[:nl]) == bad.valid == [0] * nl, (name, list(r.valid_pixels[:nl]))
    others = [k for k in range(len(init)) if k != wf.BAD_SLOT]
    _same_bits((s, reps), clean, name, nl=nl, pairs_a=others, pairs_b=others)
    _check_all([wf.no_rows_ref(name, k) for k in others], ([s[k] for k in others], [reps[k] for k in others]), "no rows, " + name)


@pytest.mark.parametrize("n_valid", wf.FEW_ROWS)
def test_rank_deficient_normal_equations_are_flagged_or_agree(n_valid):
    """test_gpu_round3.py's case on this form at 82x100: the source has valid depth at `n_valid` pixels only, in tiles of
    their own with one in the 8-pixel last tile.  Below six rows both sides divide rounding noise by rounding noise (the
    oracle with a pivoted LU, the device with LDL^T) and what is guaranteed is the flag: PAIR_RANK_DEFICIENT whenever the
    last iteration filled fewer than six rows, PAIR_NONFINITE when the state is not finite.  With 40 rows both sides agree
    to 1e-7 (40 rows: conditioned well enough, not as well as 8 200)."""
    p = wf.few_rows_pair(n_valid)
    ref = wf.few_rows_ref(n_valid)
    es, eits, tr = ref.state, ref.its, ref.trace
    ncfg, _ = wf.cfgs([wf.FEW_ITERS])
    with _engine(ncfg, p["K"], wf.STOP_SIZE) as e:
        _upload(e, p)
        s, reps = _align(e, [0] * wf.FEW_COPIES, [1] * wf.FEW_COPIES)
    assert all(np.array_equal(s[0], s[k], equal_nan=True) for k in range(wf.FEW_COPIES))
    assert tr[0]["valid_pixels"] == n_valid
    if n_valid >= 40:
        assert not wf.wild(es) and reps[0].flags == 0
        assert list(reps[0].iterations[:1]) == eits
        assert se3.state_distance(s[0], es) < 1e-7
        assert reps[0].valid_pixels[0] == tr[-1]["valid_pixels"]
    elif n_valid < 6:
        assert reps[0].flags & native.PAIR_RANK_DEFICIENT, (s[0], reps[0].flags)
        assert reps[0].valid_pixels[0] < 6
        if not np.all(np.isfinite(s[0])):
            assert reps[0].flags & native.PAIR_NONFINITE
    else:                                                          # exactly six rows: square J, invertible but fragile
        assert reps[0].flags & native.PAIR_RANK_DEFICIENT == 0 or reps[0].valid_pixels[0] < 6
        assert wf.wild(s[0]) == wf.wild(es) or (reps[0].flags & (native.PAIR_NONFINITE | native.PAIR_RANK_DEFICIENT))
    print(f"wide form, {n_valid} valid pixels: oracle {'garbage' if wf.wild(es) else 'finite'}, device flags {reps[0].flags}, "
          f"device state {'garbage' if wf.wild(s[0]) else 'finite'}, valid_pixels {reps[0].valid_pixels[0]}"
          + (f", pose distance {se3.state_distance(s[0], es):.3e}" if n_valid >= 40 else ""))


# ------------------------------------------------------------------------------------------------------------------------
# 5. exact half-pixel projections
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,sign,pairs", wf.HALF_CELLS,
                         ids=[f"{wf.size_id(s)}-{'plus' if g > 0 else 'minus'}-{n}" for s, g, n in wf.HALF_CELLS])
def test_exact_half_pixel_projections_through_this_forms_round(size, sign, pairs):
    """synthetic.half_pixel_problem: every projected coordinate is an exact half, where C round() -- half away from zero --
    decides the target of every source pixel at once.  tests/test_gpu_parity.py runs it through the level kernels (its
    "WIDE" is their 1024-thread geometry); here it goes through k_wide_pass1's own round() and row / column recovery, at 3
    tiles and at 9 with 8 pixels in the last: (w - 1)(h - 1) valid pixels exactly and the oracle's first step."""
    K, planes, state, ref = wf.half_pixel(size, sign)
    ncfg, _ = wf.cfgs([1])
    with _engine(ncfg, K, size) as e:
        e.set_level_planes(0, 0, intensity=planes[0][0], depth=planes[1][0])
        e.set_level_planes(1, 0, intensity=planes[2][0], grad_x=planes[3][0], grad_y=planes[4][0])
        got = _align(e, [0] * pairs, [1] * pairs, np.tile(state, (pairs, 1)))
    assert ref.valid == [(size[0] - 1) * (size[1] - 1)]
    _check_all([ref] * pairs, got, f"half pixels {wf.size_id(size)} sign {sign:+.0f}")
    _same_bits(got, got, size, pairs_a=range(pairs), pairs_b=[0] * pairs)


# ------------------------------------------------------------------------------------------------------------------------
# 6. narrow strips
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ef.STRIPS, ids=wf.size_id)
def test_narrow_strips(size):
    """The strips of ef.STRIPS (one to five pixels wide, and 75x53), no Huber weights, three initial states, three
    iterations: W = 1 ... 5 through this form's row / column recovery.  Where the oracle stays finite the device is held to
    Expect; where it loses its state, to the oracle's trace up to that iteration (extension_forms.check_strip).  All 18
    cases run (tests/test_wide_form_cpu.py: at least 8 of them are finite on the oracle)."""
    p, states, planes = wf.strip_case(size)
    ncfg, ocfg = ef.configs([wf.STRIP_ITERS])
    with _engine(ncfg, p["K"], size) as e:
        _upload(e, p)
        i0, d0, _, _ = e.get_level_planes(0, 0)
        i1, _, gx, gy = e.get_level_planes(1, 0)
        for got, want in zip((i0, d0, i1, gx, gy), planes):           # the device holds exactly the planes the oracle runs on
            assert np.array_equal(got, want[0], equal_nan=True), size
        s, reps = _align(e, [0] * 3, [1] * 3, np.stack(states))
    worst, finite = 0.0, 0
    for k, init in enumerate(states):
        ex = ef.expect(ocfg, p["K"], planes, init)
        print(f"wide form strip {size} state {k}: device {s[k]} iterations {list(reps[k].iterations[:1])} valid "
              f"{list(reps[k].valid_pixels[:1])} flags {reps[k].flags}; oracle {ex.state} iterations {ex.its} valid {ex.valid}")
        ef.check_strip(ex, ocfg, p["K"], planes, init, None, s[k], reps[k], (size, k))
        worst = max(worst, ef.ratio(s[k], ex))
        finite += ex.finite
    print(f"wide form strips {wf.size_id(size)}: {finite} of 3 finite on the oracle, worst pose distance / bar {worst:.3e}")
