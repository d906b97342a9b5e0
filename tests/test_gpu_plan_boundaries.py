"""Every launch geometry at the first and the last level size it takes (run with -m gpu on an MI355X), through the C ABI
against the CPU references.

The shapes are those of tests/plan_boundaries.py: levels whose LDS block is full to the last few bytes, with no chunk, one
chunk or every chunk of depth parked, and the smallest levels of the next form.  tests/test_plan_boundaries_cpu.py
vouches for the tables and for every case's reference (finite, cond(J^T J) < 1e5, one ulp of fx moves it by less than a
quarter of the bar) without a GPU.  Every case here asserts two things:

* the library's choice equals the restated planner's -- level_launch_info for the photometric aligner, the kind, threads
  and lds_bytes of last_launches() for every objective -- so that a planner constant that moves fails loudly instead of
  turning the case into an interior shape;
* the result: iteration counts identical, state_distance < 1e-9, gradient norm within 1e-9 relative, the valid pixels of
  the last iteration equal to the reference's, flags == 0; nine copies of a pair all the same bits, and on forms with the
  owner map in LDS one pair alone the same bits too.

Each case prints its largest pose distance before it asserts (DESIGN.md section 4 tables them).
"""
import numpy as np
import pytest

import plan_boundaries as pb
import test_gpu_trust_region as gtr

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3

pytestmark = pytest.mark.gpu

POSE_TOL = pb.POSE_TOL
COPIES = 9
IDS = pb.size_id


# ------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------
def _engine(ncfg, p, ext=None, objective=None):
    h, w = p["gray0"].shape
    e = odometry.AlignmentEngine(0)
    if ext is not None:
        e.set_extensions(ext)
    e.set_config(ncfg)
    e.set_intrinsic_matrix(p["K"])
    if objective is not None:
        e.set_objective(objective)
    e.reserve_frames(2, w, h)
    return e


def _upload(e, p, target_depth=False):
    e.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
    e.upload_frame(1, p["gray1"], p["depth1"] if target_depth else None, roles=native.ROLE_TARGET)


def _align(e, n_pairs, init=None):
    inits = None if init is None else np.tile(np.asarray(init, dtype=np.float64), (n_pairs, 1))
    return e.align_pairs([0] * n_pairs, [1] * n_pairs, init_states=inits, want_reports=True)


def _launches(e):
    return [(r["kind"], r["threads"], r["lds_bytes"]) for r in e.last_launches()]


def _info_matches(info, plan, what):
    got = (info["threads"], info["lds_bytes"], info["owner_in_lds"], info["source_in_lds"])
    assert got == (plan["threads"], plan["lds_bytes"], plan["owner_in_lds"], plan["source_in_lds"]), (what, info, plan)


def _check(ref, states, reps, what, flags=(0,)):
    """Every pair of a launch against the reference; every copy the same bits.  Returns the pose distance."""
    nl = len(ref.its)
    d = max(se3.state_distance(s, ref.state) for s in states)
    print(f"boundary {what}: pose distance {d:.3e}")
    for k in range(len(states)):
        assert list(reps[k].iterations[:nl]) == ref.its, (what, k, list(reps[k].iterations[:nl]), ref.its)
        assert list(reps[k].valid_pixels[:nl]) == ref.valid, (what, k, list(reps[k].valid_pixels[:nl]), ref.valid)
        assert reps[k].flags in flags, (what, k, reps[k].flags)
        assert abs(reps[k].gradient_norm - ref.gnorm) <= pb.GRAD_TOL * max(1.0, ref.gnorm), (what, k)
        assert np.array_equal(states[k], states[0]), (what, k)
        assert reps[k].gradient_norm == reps[0].gradient_norm, (what, k)
    assert d < POSE_TOL, (what, d)
    return d


def _same_bits(a, b, what):
    (sa, ra), (sb, rb) = a, b
    assert np.array_equal(sa[0], sb[0]) and ra[0].gradient_norm == rb[0].gradient_norm, what


# ------------------------------------------------------------------------------------------------------------------------
# photometric, one level per launch
# ------------------------------------------------------------------------------------------------------------------------
def _rows(table):
    return [(size, iters) for size, row in table.items() for iters in row["iters"]]


def _row_id(v):
    return pb.size_id(v) if isinstance(v, tuple) else f"it{v}"


def _single_level_case(size, iters, row, plan, what, ext=None, ref=None, stored=None):
    """The table's form, the restatement's plan and the library's choice agree; nine copies and one pair alone match the
    reference."""
    n = size[0] * size[1]
    p = pb.pair(*size)
    ncfg, _ = pb.cfgs([iters])
    assert (plan["form"], plan["threads"]) == (row["form"], row["threads"]), (what, plan)
    if row["parked"] is not None:
        assert plan["parked"] == pb.parked_count(row, n), (what, plan)
    with _engine(ncfg, p, ext=ext) as e:
        _info_matches(e.level_launch_info(0), plan, what)
        _upload(e, p)
        if stored is not None:                  # the device holds exactly the planes the reference ran on
            i0, d0, _, _ = e.get_level_planes(0, 0)
            i1, _, gx, gy = e.get_level_planes(1, 0)
            assert all(np.array_equal(a, b[0]) for a, b in zip((i0, d0, i1, gx, gy), stored)), what
        many = _align(e, COPIES)
        assert e.last_launches()[0]["workgroups"] == COPIES
        assert _launches(e) == [("persistent", plan["threads"], plan["lds_bytes"])], (what, e.last_launches())
        one = _align(e, 1)
        assert _launches(e) == [("persistent", plan["threads"], plan["lds_bytes"])], (what, e.last_launches())
    _check(ref, *many, what)
    _same_bits(many, one, what)


@pytest.mark.parametrize("size,iters", _rows(pb.PHOTO), ids=_row_id)
def test_photometric_throughput_rows(size, iters):
    """fp64 planes, throughput launch (gn_plan_level): SOLO, QUAD, MID and WIDE at their first and last sizes."""
    row = pb.PHOTO[size]
    plan = pb.plan_level(size[0] * size[1])
    _single_level_case(size, iters, row, plan, f"photometric {row['form']} {IDS(size)} parked {plan['parked']} it{iters}",
                       ref=pb.photo_ref(size, iters))


@pytest.mark.parametrize("size,iters", _rows(pb.NARROW), ids=_row_id)
def test_fp32_planes_take_mid_up_to_its_lds_limit(size, iters):
    """fp32 storage (bound_by_bytes false): 151x128 is the last MID, with nothing parked -- the size that is also the fused
    launch's limit -- and 192x101 the first WIDE chunk; against the oracle on exactly the planes the device holds."""
    row = pb.NARROW[size]
    plan = pb.plan_level(size[0] * size[1], bound_by_bytes=False)
    _, ocfg = pb.cfgs([iters])
    _single_level_case(size, iters, row, plan, f"photometric fp32 {row['form']} {IDS(size)} parked {plan['parked']} it{iters}",
                       ext=native.make_extensions(plane_storage=native.STORAGE_F32),
                       ref=pb.photo_ref(size, iters, storage=native.STORAGE_F32),
                       stored=pb.storage_planes(ocfg, pb.pair(*size), native.STORAGE_F32))


@pytest.mark.parametrize("size,iters", _rows(pb.NARROW), ids=_row_id)
def test_huber_weights_on_fp64_planes_at_the_same_sizes(size, iters):
    """fp64 planes with Huber weights: the planner is asked with bound_by_bytes TRUE (the storage alone decides it), so
    both sizes are WIDE launches that park 152 and 151 chunks -- not the MID launch at its limit, which fp32 planes, the
    latency forms and the fused geometry reach."""
    n = size[0] * size[1]
    plan = pb.plan_level(n)
    row = dict(form="WIDE", threads=1024, parked={19328: 152, 19392: 151}[n])
    _single_level_case(size, iters, row, plan, f"photometric huber {plan['form']} {IDS(size)} parked {plan['parked']} it{iters}",
                       ext=native.make_extensions(huber_delta=[pb.HUBER_DELTA]), ref=pb.photo_ref(size, iters, huber=True))


@pytest.mark.parametrize("n_pairs", [1, 8])
@pytest.mark.parametrize("size", list(pb.LATENCY), ids=IDS)
def test_latency_forms(size, n_pairs):
    """phovo_engine_set_latency_forms(1) with the wide form off, one and eight pairs: prefer_latency skips SOLO and QUAD
    -- TINY with the source in LDS at 64x32, MID at 50x41 and at its limit 151x128, WIDE at 192x101."""
    row = pb.LATENCY[size]
    plan = pb.plan_level(size[0] * size[1], prefer_latency=True)
    assert (plan["form"], plan["threads"], plan["source_in_lds"]) == (row["form"], row["threads"], row["source_in_lds"])
    p = pb.pair(*size)
    ncfg, _ = pb.cfgs([3])
    what = f"photometric latency {row['form']} {IDS(size)} parked {plan['parked']} pairs{n_pairs}"
    with _engine(ncfg, p) as e:
        e.set_latency_forms(True)
        e.set_wide_policy(-1)
        _upload(e, p)
        got = _align(e, n_pairs)
        assert _launches(e) == [("persistent", plan["threads"], plan["lds_bytes"])], (what, e.last_launches())
    _check(pb.photo_ref(size, 3), *got, what)


# ------------------------------------------------------------------------------------------------------------------------
# levels beyond LDS
# ------------------------------------------------------------------------------------------------------------------------
def test_first_level_beyond_lds():
    """200x194 = 38 800 pixels, one chunk more than WIDE takes.  40 pairs: the sliding-window kernel and the exact kernel
    behind it, two runs bit-equal; with the slide policy -1 the exact kernel alone, the LDS part of whose owner map ends at
    38 592 and leaves 208 pixels in HBM; one pair whose initial state leaves the window at once is finished by the exact
    kernel, flagged, with the oracle's result."""
    size = pb.BEYOND
    plan = pb.plan_level(size[0] * size[1])
    assert plan["form"] == "HUGE" and plan["owner_lds_entries"] == pb.BEYOND_SEAM and not plan["mask_in_hbm"]
    p = pb.pair(*size)
    ncfg, _ = pb.cfgs([3])
    exact_launch = (plan["threads"], plan["lds_bytes"])
    with _engine(ncfg, p) as e:
        e.set_wide_policy(-1)
        info = e.level_launch_info(0)
        assert not info["owner_in_lds"] and info["threads"] == 768, info          # the sliding-window kernel runs first
        _upload(e, p)
        slide = _align(e, 40)
        ls = _launches(e)
        assert [l[0] for l in ls] == ["slide", "slide_fallback"] and ls[0][1] == 768 and ls[1][1:] == exact_launch, ls
        slide2 = _align(e, 40)
        left = _align(e, 1, init=pb.LEAVES_WINDOW)
        ls = _launches(e)
        assert [l[0] for l in ls] == ["slide", "slide_fallback"] and ls[1][1:] == exact_launch, ls
        e.set_slide_policy(-1)
        _info_matches(e.level_launch_info(0), plan, size)
        exact = _align(e, 40)
        assert _launches(e) == [("persistent",) + exact_launch], e.last_launches()
        left_exact = _align(e, 1, init=pb.LEAVES_WINDOW)
    ref = pb.photo_ref(size, 3)
    assert np.array_equal(slide[0], slide2[0])
    _check(ref, *slide, f"photometric slide {IDS(size)} pairs40", flags=(0, native.PAIR_WINDOW_FALLBACK))
    _check(ref, *exact, f"photometric HUGE {IDS(size)} seam {plan['owner_lds_entries']} pairs40")
    ref_left = pb.photo_ref(size, 3, init=pb.LEAVES_WINDOW)
    _check(ref_left, *left, f"photometric handover {IDS(size)}", flags=(native.PAIR_WINDOW_FALLBACK,))
    _check(ref_left, *left_exact, f"photometric HUGE {IDS(size)} from the handover state")
    assert np.array_equal(left[0], left_exact[0])           # it left in its first iteration: the exact kernel did all of it


@pytest.mark.parametrize("size", list(pb.EXACT), ids=IDS)
def test_exact_kernel_where_the_ballots_move_to_hbm(size):
    """928x668 (9686 chunks) is the last size whose ballots fill their half of LDS, 800x775 (9688 chunks) keeps them in
    HBM: the exact kernel alone, two pairs, two iterations; and one pair handed over from the sliding window."""
    n = size[0] * size[1]
    plan = pb.plan_level(n)
    assert plan["form"] == "HUGE" and plan["mask_in_hbm"] == pb.EXACT[size]["mask_in_hbm"]
    p = pb.pair(*size)
    ncfg, _ = pb.cfgs([pb.EXACT_ITERS])
    exact_launch = (plan["threads"], plan["lds_bytes"])
    ballots = "hbm" if plan["mask_in_hbm"] else "lds"
    with _engine(ncfg, p) as e:
        e.set_wide_policy(-1)
        e.set_slide_policy(-1)
        _info_matches(e.level_launch_info(0), plan, size)
        _upload(e, p)
        exact = _align(e, 2)
        assert _launches(e) == [("persistent",) + exact_launch], e.last_launches()
        e.set_slide_policy(0)
        left = _align(e, 1, init=pb.LEAVES_WINDOW)
        ls = _launches(e)
        assert [l[0] for l in ls] == ["slide", "slide_fallback"] and ls[1][1:] == exact_launch, ls
    _check(pb.photo_ref(size, pb.EXACT_ITERS), *exact, f"photometric HUGE {IDS(size)} ballots {ballots}")
    _check(pb.photo_ref(size, pb.EXACT_ITERS, init=pb.LEAVES_WINDOW), *left,
           f"photometric handover {IDS(size)} ballots {ballots}", flags=(native.PAIR_WINDOW_FALLBACK,))


# ------------------------------------------------------------------------------------------------------------------------
# fused runs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", list(pb.FUSED), ids=IDS)
def test_fused_runs_at_the_limits_of_fusability(base):
    """Levels 1 and 2 of four bases: the largest level exactly at the fused launch's LDS limit, one chunk beyond it, the
    smallest level in the first fusable chunk and one pixel count below it.  FUSION_AUTO, FUSION_SPLIT and FUSION_OFF:
    launch kinds, threads and LDS as the restated planner gives them, AUTO and SPLIT bit-identical where a fused launch
    exists, all modes within the bar of the oracle with equal iteration counts."""
    row = pb.FUSED[base]
    ns = [w * h for w, h in row["levels"]][::-1]                  # coarse to fine
    p = pb.fused_pair(*base)
    ncfg, _ = pb.cfgs(pb.FUSED_MAX_ITER, pb.FUSED_MIN_GRAD)
    out, launches = {}, {}
    modes = (native.FUSION_AUTO, native.FUSION_SPLIT, native.FUSION_OFF)
    with _engine(ncfg, p) as e:
        _upload(e, p)
        assert e.level_size(1) == row["levels"][0] and e.level_size(2) == row["levels"][1]
        for mode in modes:
            e.set_level_fusion(mode)
            out[mode] = _align(e, pb.FUSED_COPIES)
            launches[mode] = _launches(e)
    for mode in modes:
        assert launches[mode] == pb.expected_launches(ns, mode), (base, mode, launches[mode])
    assert (launches[native.FUSION_AUTO][0][0] == "fused") == row["fused"], launches
    assert ("fused" in [l[0] for m in modes for l in launches[m]]) == row["fused"]
    ref = pb.fused_ref(base)
    for mode, name in zip(modes, ("auto", "split", "off")):
        _check(ref, *out[mode], f"photometric fused-{name} {IDS(base)} its {ref.its}")
    if row["fused"]:
        a, s = out[native.FUSION_AUTO], out[native.FUSION_SPLIT]
        assert np.array_equal(a[0], s[0])
        assert all(x.gradient_norm == y.gradient_norm and list(x.valid_pixels[:3]) == list(y.valid_pixels[:3])
                   for x, y in zip(a[1], s[1]))


# ------------------------------------------------------------------------------------------------------------------------
# bi-objective and trust region
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(pb.BI), ids=IDS)
def test_biobjective_forms(size):
    """256 threads x 2 workgroups per CU up to 81 880 of 81 920 bytes, 512 x 1 up to 163 688 of 163 840, the owner map in
    HBM beyond: each form's last size and the next form's first, against tests/biobjective_ref.py."""
    row = pb.BI[size]
    plan = pb.plan_biobjective(size[0] * size[1])
    assert (plan["form"], plan["threads"]) == (row["form"], row["threads"]) and row["lds_bytes"] in (None, plan["lds_bytes"])
    p = pb.bi_pair(*size)
    ncfg, _ = pb.bi_cfgs()
    what = f"biobjective {row['form']} {IDS(size)} lds {plan['lds_bytes']}"
    with _engine(ncfg, p, objective=native.OBJECTIVE_BIOBJECTIVE) as e:
        _upload(e, p, target_depth=True)
        many = _align(e, COPIES)
        assert _launches(e) == [("biobjective", plan["threads"], plan["lds_bytes"])], (what, e.last_launches())
        one = _align(e, 1)
    _check(pb.bi_ref(size), *many, what)
    if plan["owner_in_lds"]:
        _same_bits(many, one, what)


@pytest.mark.parametrize("size", list(pb.TR), ids=IDS)
def test_trust_region_forms(size):
    """The same three forms with a fixed block 432 bytes larger: 81 784 and 163 696 bytes at the last sizes; against
    tests/trust_region_ref.py under the rules of tests/test_gpu_trust_region.py (steps, accepted steps, terminations, rows,
    costs, radius, gradient norm) and the pose bar."""
    row = pb.TR[size]
    plan = pb.plan_trust_region(size[0] * size[1])
    assert (plan["form"], plan["threads"]) == (row["form"], row["threads"]) and row["lds_bytes"] in (None, plan["lds_bytes"])
    p = pb.tr_pair(*size)
    cfg, opt = pb.tr_cfg()
    what = f"trust_region {row['form']} {IDS(size)} lds {plan['lds_bytes']}"
    ref = pb.tr_ref(size)
    with gtr._engine(cfg, opt, p["K"]) as e:
        gtr._upload(e, [p])
        states, reps = _align(e, COPIES, init=pb.TR_INIT)
        tr = e.trust_region_reports(COPIES)
        assert _launches(e) == [("trust_region", plan["threads"], plan["lds_bytes"])], (what, e.last_launches())
        one = _align(e, 1, init=pb.TR_INIT)
        tr_one = e.trust_region_reports(1)
    d = max(se3.state_distance(s, ref.state) for s in states)
    print(f"boundary {what}: pose distance {d:.3e}")
    for k in range(COPIES):
        gtr.compare_pair(k, states[k], reps[k], tr, ref.state, ref.recs, cfg.num_levels)
        assert reps[k].flags == 0
        assert np.array_equal(states[k], states[0]) and np.array_equal(tr[k:k + 1], tr[0:1]), (what, k)
    assert d < POSE_TOL, (what, d)
    if plan["owner_in_lds"]:
        assert np.array_equal(one[0][0], states[0]) and np.array_equal(tr_one, tr[0:1]), what
