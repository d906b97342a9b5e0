"""The sliding-window kernel (csrc/gn_slide_kernel.hip) at the exact edges of its window (run with -m gpu on an MI355X).

The inputs are those of tests/slide_window.py: targets in the last slot the window admits and one pixel beyond it, ahead
of the source's band and behind it, with the ring full (m = M_MAX) and with slack (m = 4); sources of two depths that
collide on such targets; a rotation that reaches both edges in one iteration; a pair that leaves at a later iteration;
inside pairs drawn by a workgroup straight after a voided one; narrow storages and Huber weights.
tests/test_slide_window_cpu.py vouches for every fixture without a GPU (which pair must leave the window, margins from
every rounding boundary, cond(J^T J) <= 1e5, one ulp of fx).

Every case is held to oracle.optimize on the planes the device holds, from the fixture's start state: iteration counts and
the last iteration's valid pixels exact, state_distance < POSE_TOL, gradient norm within 1e-9 relative, and the flag the CPU
predicts -- 0 or PAIR_WINDOW_FALLBACK, never "either".  Every case also asserts the launches ("slide", "slide_fallback")
and that the level is planned with 768 threads and no owner map in LDS.  A pair that left in its first iteration is
bit-equal to the same pair under set_slide_policy(-1); one that stayed is held to the exact kernel by the bar only (the two
forms keep different expressions).

Each case prints its pose distance over the bar before it asserts (DESIGN.md section 4 tables them).
"""
import numpy as np
import pytest

import slide_window as sw
from test_gpu_parity import POSE_TOL

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3

pytestmark = pytest.mark.gpu

GRAD_TOL = sw.GRAD_TOL
KINDS = ["slide", "slide_fallback"]


# ------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------
def _engine(fx_, n_frames=2):
    w, h = fx_.size
    e = odometry.AlignmentEngine(0)
    ext = fx_.extensions()
    if ext is not None:
        e.set_extensions(ext)
    e.set_config(fx_.cfgs()[0])
    e.set_intrinsic_matrix(fx_.p["K"])
    e.set_depth_range(sw.MIN_DEPTH, sw.MAX_DEPTH)
    e.set_wide_policy(-1)                        # a handful of pairs would take the wide form: the batch forms, as a batch takes them
    e.reserve_frames(n_frames, w, h)
    info = e.level_launch_info(0)
    assert info["threads"] == sw.SLIDE_THREADS and not info["owner_in_lds"], (fx_.name, info)
    return e


def _upload(e, fx_, src=0, tgt=1):
    e.upload_frame(src, fx_.p["gray0"], fx_.p["depth0"], roles=native.ROLE_SOURCE)
    if tgt is not None:
        e.upload_frame(tgt, fx_.p["gray1"], None, roles=native.ROLE_TARGET)
    # the device holds exactly the planes the reference ran on
    i0, d0, _, _ = e.get_level_planes(src, 0)
    stored = fx_.planes()
    assert np.array_equal(i0, stored[0][0]) and np.array_equal(d0, stored[1][0]), fx_.name
    if tgt is not None:
        i1, _, gx, gy = e.get_level_planes(tgt, 0)
        assert all(np.array_equal(a, b[0]) for a, b in zip((i1, gx, gy), stored[2:])), fx_.name


def _align(e, fx_, n_pairs=1, slide=True):
    inits = np.tile(fx_.init, (n_pairs, 1))
    out = e.align_pairs([0] * n_pairs, [1] * n_pairs, init_states=inits, want_reports=True)
    kinds = [r["kind"] for r in e.last_launches()]
    assert kinds == (KINDS if slide else ["persistent"]), (fx_.name, kinds)
    return out


def _check(fx_, states, reps, what=None):
    """Every pair of a launch against the fixture's reference, with the predicted flag; returns distance / bar."""
    ref = sw.ref(fx_)
    what = what or fx_.name
    d = max(se3.state_distance(s, ref.state) for s in states)
    print(f"slide window {what}: flag {ref.flags} pose distance / bar {d / POSE_TOL:.3e}")
    for k in range(len(states)):
        assert list(reps[k].iterations[:1]) == ref.its, (what, k, list(reps[k].iterations[:1]), ref.its)
        assert list(reps[k].valid_pixels[:1]) == ref.valid, (what, k, list(reps[k].valid_pixels[:1]), ref.valid)
        assert reps[k].flags == ref.flags, (what, k, reps[k].flags, ref.flags)
        assert abs(reps[k].gradient_norm - ref.gnorm) <= GRAD_TOL * max(1.0, ref.gnorm), (what, k)
    assert d < POSE_TOL, (what, d)
    return d / POSE_TOL


def _same_bits(a, b, what):
    (sa, ra), (sb, rb) = a, b
    assert len(sa) == len(sb)
    for k in range(len(sa)):
        assert np.array_equal(sa[k], sb[k]) and ra[k].gradient_norm == rb[k].gradient_norm, (what, k)
        assert ra[k].flags == rb[k].flags and list(ra[k].valid_pixels[:1]) == list(rb[k].valid_pixels[:1]), (what, k)


def _one_pair_case(fx_):
    """One pair through the sliding-window launch and its follow-up; a second enqueue gives the same bits; a pair that
    left in its first iteration is bit for bit what the exact kernel does alone."""
    ref = sw.ref(fx_)
    with _engine(fx_) as e:
        _upload(e, fx_)
        got = _align(e, fx_)
        again = _align(e, fx_)
        e.set_slide_policy(-1)
        exact = _align(e, fx_, slide=False)
    _check(fx_, *got)
    _same_bits(got, again, fx_.name)
    assert exact[1][0].flags == 0 and list(exact[1][0].iterations[:1]) == ref.its, fx_.name
    assert se3.state_distance(exact[0][0], ref.state) < POSE_TOL, fx_.name
    if ref.leaves_at == 0:
        assert np.array_equal(got[0][0], exact[0][0]) and got[1][0].gradient_norm == exact[1][0].gradient_norm, fx_.name


# ------------------------------------------------------------------------------------------------------------------------
# A. the one-pixel boundary, one iteration
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["limit", "beyond"])
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("size", list(sw.SHAPES), ids=sw.size_id)
def test_one_pixel_boundary(size, direction, where):
    """A uniform displacement of m bands ahead (m - 1 behind) puts a valid target in the window's last (first) slot and
    none outside: flags == 0.  One pixel further a handful of pixels are outside: PAIR_WINDOW_FALLBACK, and the exact kernel
    does the whole pair."""
    fx_ = sw.boundary(size, direction, where)
    assert sw.ref(fx_).flags == (0 if where == "limit" else native.PAIR_WINDOW_FALLBACK)
    _one_pair_case(fx_)


@pytest.mark.parametrize("where", ["limit", "beyond"])
@pytest.mark.parametrize("size,direction", [(s, d) for s, row in sw.ALTERNATIVES.items() for d in row],
                         ids=lambda v: sw.size_id(v) if isinstance(v, tuple) else v)
def test_one_pixel_boundary_written_so_that_residuals_count(size, direction, where):
    """200x194 forward and 640x480 backward once more, the same limits written with other rows and columns.  As the issue's
    table writes them no target is itself a valid source pixel, no residual reaches the sums and the cases above test the
    flag and the valid count only; written this way tens of thousands of the owners in the edge band decide the result."""
    fx_ = sw.boundary(size, direction, where, alternative=True)
    assert sw.ref(fx_).flags == (0 if where == "limit" else native.PAIR_WINDOW_FALLBACK) and sw.ref(fx_).gnorm > 0.0
    _one_pair_case(fx_)


# ------------------------------------------------------------------------------------------------------------------------
# B. ring full with collisions
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("size", list(sw.TWO_DEPTHS), ids=sw.size_id)
def test_two_depths_collide_with_the_ring_full(size, direction):
    """Near sources on the limit and far sources a fraction as far land on the same targets, thousands of which are in the
    band at the window's edge and are valid sources themselves, so that the winner's residual reaches the sums
    (tests/test_slide_window_cpu.py counts them): the last raster writer -- forward the far source, backward the near one --
    must win while every band of the ring is live.  Eight copies in one launch and a second enqueue give the same bits --
    the ring and the ballot ring are left clean."""
    fx_ = sw.collisions(size, direction)
    assert sw.ref(fx_).flags == 0
    with _engine(fx_) as e:
        _upload(e, fx_)
        one = _align(e, fx_)
        eight = _align(e, fx_, 8)
        again = _align(e, fx_, 8)
    _check(fx_, *eight)
    _same_bits(eight, again, fx_.name)
    _same_bits(eight, ([one[0][0]] * 8, [one[1][0]] * 8), fx_.name)


# ------------------------------------------------------------------------------------------------------------------------
# C. both edges at once
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 4])
@pytest.mark.parametrize("where", ["limit", "beyond"])
def test_rotation_reaches_both_edges(where, iters):
    """An in-plane rotation about a principal point left of the centre: the right border is within a row of the forward
    limit and the left border within a row of the backward limit in the same iteration.  The flag is the OR of the
    window test over the states that enter the oracle's iterations."""
    fx_ = sw.rotation(where, iters)
    assert sw.ref(fx_).flags == (0 if where == "limit" else native.PAIR_WINDOW_FALLBACK)
    _one_pair_case(fx_)


# ------------------------------------------------------------------------------------------------------------------------
# D. leaving at a later iteration
# ------------------------------------------------------------------------------------------------------------------------
def test_pair_leaves_at_a_later_iteration():
    """Inside at the start state (on the forward limit), outside after a Gauss-Newton step of the oracle's trace: the
    sliding-window kernel completes its iterations up to there, voids the next one and the exact kernel continues from it.
    Total iterations, valid pixels, pose and flag are the oracle's."""
    fx_ = sw.leaves_later()
    ref = sw.ref(fx_)
    assert ref.leaves_at >= 1 and ref.flags == native.PAIR_WINDOW_FALLBACK
    _one_pair_case(fx_)


# ------------------------------------------------------------------------------------------------------------------------
# E. a dirty ring handed to the next pair
# ------------------------------------------------------------------------------------------------------------------------
def test_voided_iteration_leaves_nothing_to_the_next_pair():
    """520 positions on a persistent grid of 256 workgroups, alternating inside-forward, outside-forward, inside-backward,
    outside-backward: a workgroup draws an inside pair straight after an iteration that was voided with owners left in the
    ring.  Every position has the bits and the flag of its kind alone."""
    fixtures = [sw.boundary(sw.DIRTY_SIZE, d, wh) for d, wh in sw.DIRTY_KINDS]
    n_kinds = len(fixtures)
    with _engine(fixtures[0], n_frames=n_kinds + 1) as e:
        alone = []
        for i, f in enumerate(fixtures):
            _upload(e, f, src=i, tgt=n_kinds if i == 0 else None)
        for i, f in enumerate(fixtures):
            alone.append(e.align_pairs([i], [n_kinds], init_states=f.init[None, :], want_reports=True))
        which = [k % n_kinds for k in range(sw.DIRTY_POSITIONS)]
        inits = np.stack([fixtures[c].init for c in which])
        states, reps = e.align_pairs(which, [n_kinds] * len(which), init_states=inits, want_reports=True)
        assert [r["kind"] for r in e.last_launches()] == KINDS
        assert e.last_launches()[0]["workgroups"] < sw.DIRTY_POSITIONS // 2
    for i, f in enumerate(fixtures):
        _check(f, *alone[i], what=f"dirty ring, alone, {f.name}")
    for k, c in enumerate(which):
        assert np.array_equal(states[k], alone[c][0][0]), (k, c)
        assert reps[k].flags == alone[c][1][0].flags == sw.ref(fixtures[c]).flags, (k, c, reps[k].flags)
        assert reps[k].gradient_norm == alone[c][1][0].gradient_norm, (k, c)
        assert list(reps[k].valid_pixels[:1]) == list(alone[c][1][0].valid_pixels[:1]), (k, c)
        assert list(reps[k].iterations[:1]) == [1], (k, c)


# ------------------------------------------------------------------------------------------------------------------------
# F. storage and Huber
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["limit", "beyond"])
@pytest.mark.parametrize("cell", sw.STORAGE_CELLS, ids=["f32", "f16", "huber"])
def test_storage_and_huber_at_the_forward_limit(cell, where):
    """The window logic is one piece of code compiled three times (fp64, fp32, fp16 planes), and the Huber weights are a
    second copy of pass 2: each at the 800x50 forward limit and one pixel beyond, against the identically extended oracle
    on the stored planes."""
    storage, huber = cell
    fx_ = sw.boundary((800, 50), "forward", where, storage=storage, huber=huber)
    assert sw.ref(fx_).flags == (0 if where == "limit" else native.PAIR_WINDOW_FALLBACK)
    _one_pair_case(fx_)
