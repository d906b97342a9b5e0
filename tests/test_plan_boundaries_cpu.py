"""CPU pre-checks of tests/plan_boundaries.py: the tables name the sizes they claim to name, and every case of
tests/test_gpu_plan_boundaries.py is well-posed for the flat 1e-9 pose bar on its reference.

* every "last" shape is accepted by the restated planner in its form and the next chunk count is not (for the bi-objective
  and the trust region, whose owner term is 4 n and not chunk-granular, the named neighbour shape takes that place); every
  "first" shape lies in the first chunk, or is the named neighbour, of its form; the parked counts are exactly 0, 1, all or
  all but two as the table says; the pyramid levels of the fused bases are those listed;
* every case is finite on its reference, cond(J^T J) stays below 1e5 at every iteration, one ulp of fx moves the result
  by less than a quarter of the bar and changes no iteration count (the guard of tests/test_extensions_cpu.py), and on the
  fused bases no gradient norm of the trace lies within 0.5 % of a threshold.
"""
import numpy as np
import pytest

import plan_boundaries as pb
import pyramid_exact

from phovo_amd import native

IDS = pb.size_id


def _n(size):
    return size[0] * size[1]


def _form(n, **kw):
    p = pb.plan_level(n, **kw)
    return p and p["form"]


# ------------------------------------------------------------------------------------------------------------------------
# the restatement and the tables
# ------------------------------------------------------------------------------------------------------------------------
def test_the_restated_sums_are_the_hand_formulas():
    for t in (64, 256, 512, 1024):
        assert pb.lds_fixed_bytes(t) == 8 * (40 + 32 * t // 64) + 16
        assert pb.tr_lds_fixed_bytes(t) == pb.lds_fixed_bytes(t) + 8 * 50 + 4 * 8 == pb.lds_fixed_bytes(t) + 432
    for n in (1, 63, 64, 65, 2048, 2050, 19328):
        assert pb.owner_lds_entries(n, 512) == -(-n // 64) * 64 + 512
    assert pb.LDS_LIMIT == 163840 and pb.CHUNK_BYTES == 512


def _check_row(size, row, **kw):
    n, c = _n(size), pb.chunks(_n(size))
    p = pb.plan_level(n, **kw)
    assert (p["form"], p["threads"]) == (row["form"], row["threads"]), (size, p)
    assert p["owner_in_lds"] and not p["source_in_lds"]
    if row["parked"] is not None:
        assert p["parked"] == pb.parked_count(row, n), (size, p["parked"])
    # lds_bytes is the used bytes rounded up to 8 plus whole parked chunks, inside the form's share of LDS
    used = (pb.lds_fixed_bytes(p["threads"]) + 4 * pb.owner_lds_entries(n, p["threads"]) + 7) & ~7
    assert p["lds_bytes"] == used + 512 * p["parked"] <= pb.LDS_LIMIT // p["wgs_per_cu"]
    if p["parked"] < c:                                         # not everything parked: no room for one chunk more
        assert pb.LDS_LIMIT // p["wgs_per_cu"] - p["lds_bytes"] < 512
    if row["edge"] == "last":
        assert _form(64 * c, **kw) == row["form"]              # the whole chunk count is accepted ...
        assert _form(64 * c + 1, **kw) != row["form"], size    # ... and c + 1 chunks are not
    if row["edge"] == "first":
        assert _form(64 * (c - 1) + 1, **kw) == row["form"]    # the whole chunk count takes the form ...
        assert _form(64 * (c - 1), **kw) != row["form"], size  # ... and c - 1 chunks do not
    return p


@pytest.mark.parametrize("size", list(pb.PHOTO), ids=IDS)
def test_photometric_rows(size):
    row = pb.PHOTO[size]
    n, c = _n(size), pb.chunks(_n(size))
    p = _check_row(size, row)
    if size == (64, 32):
        assert n == 2048 and c == 32 and p["parked"] == 2
    if size == (50, 41):
        assert n == 2050 and c == 33                                  # the first chunk count beyond 2048 pixels
    if size == (128, 74):
        assert n == 9472 and p["parked"] == 1                         # waves 1-3 of four have no parked run
    if size == (120, 80):
        assert n == 9600 and p["parked"] == 0 and pb.LDS_LIMIT // 4 - p["lds_bytes"] == 176
    if size == (97, 99):
        assert n == 9603 and n % 64 == 3 and c == 151                 # partial last chunk
    if size == (128, 100):
        assert n == 12800 and c == 200 and p["parked"] == 51 and 4 * 51 >= c          # a quarter or more: MID stays
    if size == (134, 96):
        assert n == 12864 and c == 201 == p["parked"]
        mid = pb.plan_level(n, bound_by_bytes=False)                  # MID would park 50 of 201: under a quarter
        assert mid["form"] == "MID" and mid["parked"] == 50 and 4 * 50 < c
    if size == (129, 100):
        assert n == 12900 and c == 202 == p["parked"] and n % 64 == 36
        assert pb.plan_level(64 * c + 1)["parked"] < c + 1            # the last size with every chunk parked
    if size == (112, 116):
        assert n == 12992 and c == 203 and p["parked"] == 201 == c - 2
    if size == (202, 192):
        assert n == 38784 and c == 606 and pb.LDS_LIMIT - p["lds_bytes"] == 176


def test_levels_beyond_lds():
    n = _n(pb.BEYOND)
    p = pb.plan_level(n)
    assert n == 38800 and pb.chunks(n) == 607 and _form(64 * 606) == "WIDE"
    assert (p["form"], p["threads"], p["owner_in_lds"], p["mask_in_hbm"]) == ("HUGE", 1024, False, False)
    assert p["owner_lds_entries"] == pb.BEYOND_SEAM == 38592 and n - p["owner_lds_entries"] == 208
    assert p["lds_bytes"] <= pb.LDS_LIMIT < p["lds_bytes"] + 4 * 64   # not one chunk more of the owner map fits
    for size, row in pb.EXACT.items():
        q = pb.plan_level(_n(size))
        assert q["form"] == "HUGE" and q["mask_in_hbm"] == row["mask_in_hbm"], size
        assert 0 < q["owner_lds_entries"] < _n(size) and q["owner_lds_entries"] % 64 == 0
        assert q["lds_bytes"] <= pb.LDS_LIMIT
    assert _n((928, 668)) == 619904 and pb.chunks(619904) == 9686
    assert pb.lds_fixed_bytes(1024) + 8 * 9686 == pb.LDS_LIMIT // 2   # the ballots fill their half to the byte
    assert pb.plan_level(64 * 9686 + 1)["mask_in_hbm"]
    assert _n((800, 775)) == 620000 and pb.chunks(620000) == 9688
    assert pb.plan_level((1 << 21) - 1) is not None and pb.plan_level(1 << 21) is None


@pytest.mark.parametrize("size", list(pb.NARROW), ids=IDS)
def test_narrow_storage_rows(size):
    """fp32 planes: bound_by_bytes is false and MID runs up to its LDS limit with nothing parked.  fp64 planes with Huber
    weights go through gn_plan_level with bound_by_bytes TRUE (the engine passes the storage alone), so both shapes are
    WIDE launches there: asserted, so that the GPU module's cases are what they say."""
    p = _check_row(size, pb.NARROW[size], bound_by_bytes=False)
    if size == (151, 128):
        assert _n(size) == 19328 and pb.LDS_LIMIT // 2 - p["lds_bytes"] == 176
    assert _form(_n(size)) == "WIDE"


def test_latency_rows():
    for size, row in pb.LATENCY.items():
        p = pb.plan_level(_n(size), prefer_latency=True)
        assert (p["form"], p["threads"], p["source_in_lds"]) == (row["form"], row["threads"], row["source_in_lds"]), size
    assert pb.plan_level(2048, prefer_latency=True)["lds_bytes"] == pb.lds_fixed_bytes(256) + 4 * (2048 + 256) + 8 * 2048
    assert _form(19328 + 1, prefer_latency=True) == "WIDE"


@pytest.mark.parametrize("base", list(pb.FUSED), ids=IDS)
def test_fused_bases(base):
    row = pb.FUSED[base]
    for level in (1, 2):
        assert pyramid_exact.level_size(*base, level) == row["levels"][level - 1], (base, level)
    ns = [_n(s) for s in row["levels"]]
    assert all(pb.level_fusable(n) for n in ns) == row["fused"]
    auto = pb.expected_launches(ns[::-1], native.FUSION_AUTO)
    assert (["fused"] == [k for k, _, _ in auto]) == row["fused"], auto
    if base == (302, 256):
        assert ns[0] == 19328 and pb.level_fusable(19328) and not pb.level_fusable(19329)
        assert pb.LDS_LIMIT // 2 - pb.fused_lds_bytes(19328) == 176
        assert pb.fused_parked(19328, 19328) == 0 and pb.fused_parked(19328, ns[1]) == pb.chunks(ns[1])
    if base == (384, 202):
        assert ns[0] == 19392 and not pb.level_fusable(ns[0]) and pb.level_fusable(ns[1])
    if base == (200, 164):
        assert ns[1] == 2050 and pb.level_fusable(2049) and not pb.level_fusable(2048)
        assert pb.fused_parked(ns[0], ns[1]) == pb.chunks(ns[1])
    if base == (256, 128):
        assert ns[1] == 2048 and not pb.level_fusable(ns[1]) and pb.level_fusable(ns[0])
    if not row["fused"]:
        for mode in (native.FUSION_AUTO, native.FUSION_SPLIT, native.FUSION_OFF):
            assert [k for k, _, _ in pb.expected_launches(ns[::-1], mode)] == ["persistent", "persistent"]


@pytest.mark.parametrize("table,plan", [(pb.BI, pb.plan_biobjective), (pb.TR, pb.plan_trust_region)], ids=["bi", "tr"])
def test_objective_rows(table, plan):
    for size, row in table.items():
        p, q = plan(_n(size)), plan(_n(row["neighbour"]))
        assert (p["form"], p["threads"]) == (row["form"], row["threads"]), (size, p)
        assert q["form"] != p["form"], (size, row["neighbour"])
        assert p["owner_in_lds"] == (row["form"] != "HBM")
        if row["lds_bytes"] is not None:
            assert p["lds_bytes"] == row["lds_bytes"], (size, p["lds_bytes"])
            # the neighbour's sums in this form pass its share of LDS
            nn = _n(row["neighbour"])
            fixed = pb.lds_fixed_bytes if plan is pb.plan_biobjective else pb.tr_lds_fixed_bytes
            assert p["lds_bytes"] <= pb.LDS_LIMIT // p["wgs_per_cu"] < fixed(p["threads"]) + 8 * pb.chunks(nn) + 4 * nn


# ------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------
def _vouch(r, what):
    assert r.finite, what
    assert r.cond < pb.COND_MAX, (what, r.cond)
    sens, its = r.nudged()
    assert sens < 0.25 * pb.POSE_TOL, f"{what}: one ulp of fx moves the reference by {sens:.3e}"
    assert its == r.its, (what, its, r.its)
    return sens


@pytest.mark.parametrize("size", list(pb.PHOTO), ids=IDS)
def test_photometric_cases_are_well_posed(size):
    for iters in pb.PHOTO[size]["iters"]:
        r = pb.photo_ref(size, iters)
        assert r.its == [iters]
        _vouch(r, (size, iters))


@pytest.mark.parametrize("size", list(pb.NARROW), ids=IDS)
def test_narrow_storage_huber_and_latency_cases_are_well_posed(size):
    for iters in pb.NARROW[size]["iters"]:
        _vouch(pb.photo_ref(size, iters, storage=native.STORAGE_F32), (size, iters, "fp32"))
        _vouch(pb.photo_ref(size, iters, huber=True), (size, iters, "huber"))
    _vouch(pb.photo_ref(size, 3), (size, "latency"))           # (64x32 and 50x41: the photometric rows above)


def test_cases_beyond_lds_are_well_posed():
    _vouch(pb.photo_ref(pb.BEYOND, 3), pb.BEYOND)
    _vouch(pb.photo_ref(pb.BEYOND, 3, init=pb.LEAVES_WINDOW), (pb.BEYOND, "leaves the window"))
    for size in pb.EXACT:
        _vouch(pb.photo_ref(size, pb.EXACT_ITERS), size)
        _vouch(pb.photo_ref(size, pb.EXACT_ITERS, init=pb.LEAVES_WINDOW), (size, "handed over"))


@pytest.mark.parametrize("base", list(pb.FUSED), ids=IDS)
def test_fused_cases_are_well_posed(base):
    r = pb.fused_ref(base)
    _vouch(r, base)
    assert r.its[0] == 1 and 1 <= r.its[1] <= pb.FUSED_MAX_ITER[1] and 1 <= r.its[2] <= pb.FUSED_MAX_ITER[2]
    for level, g in r.gnorms:
        thr = pb.FUSED_MIN_GRAD[level]
        assert abs(g - thr) > pb.THRESHOLD_MARGIN * thr, (base, level, g)
    print(base, r.its, sorted(r.gnorms, key=lambda e: abs(e[1] - 120.0))[:2])


def test_fused_iteration_counts():
    """Data-dependent termination is what a fused launch is for: the thresholds stop the bases at different counts."""
    its = {base: pb.fused_ref(base).its for base in pb.FUSED}
    assert its[(302, 256)] == [1, 4, 4] and its[(200, 164)] == [1, 3, 11] and its[(256, 128)] == [1, 3, 3], its


@pytest.mark.parametrize("size", list(pb.BI), ids=IDS)
def test_biobjective_cases_are_well_posed(size):
    r = pb.bi_ref(size)
    assert r.its == [pb.OBJECTIVE_ITERS] and r.flags == 0
    _vouch(r, size)


@pytest.mark.parametrize("size", list(pb.TR), ids=IDS)
def test_trust_region_cases_are_well_posed(size):
    r = pb.tr_ref(size)
    assert r.margin > 1e-6, (size, r.margin)                   # no knife-edge decision (tests/test_gpu_trust_region.py)
    assert all(rec["noise_from"] is None for rec in r.recs.values())
    rec = r.recs[0]
    assert rec["steps"] == pb.TR_STEPS and 2 <= rec["accepted"] < rec["steps"]      # accepted and rejected steps
    _vouch(r, size)
