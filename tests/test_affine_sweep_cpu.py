"""CPU side of the affine-illumination kernel's randomised sweep (tests/tools/fuzz_objectives.py, mode `affine`;
tests/test_gpu_affine_sweep.py runs it on the device).  No GPU.

* The draws of the three older modes are what they were before `affine` was added: case_key of 50 cases per mode, flag and
  seed against digests computed at the commit before (the replays of test_gpu_objective_sweeps.TR_REPLAYS name cases by
  seed and number).
* The committed sweeps (fuzz_objectives.AFFINE_SWEEPS) reach every class coverage() knows, with exactly their seeds and
  counts.
* The checker alone, on oracle-built pyramids in place of the device's, stays inside the caps on the plain sweep: the 5 %
  the GPU test allows to be set aside cannot be filled by inputs on which the checker itself is unstable, most cases are
  held to the flat bar, and both ways a level can end are there."""
import collections
import concurrent.futures as cf
import hashlib
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import fuzz_objectives as fo  # noqa: E402

# sha256 of "\n".join(case_key) over draw_cases(50, seed, mode, flags), computed at the parent of the commit that added `affine`
OLD_DRAWS = {
    ("bi", (), 5): "57ea377d55def044fff0798076ebe09d1263b2092617d448991232dad91d9d32",
    ("bi", (), 12): "2c964aeb804cfd999f4f559f048d4dddd00d5ff15705e0988d6b24e71a27f885",
    ("bi", ("big",), 5): "b6e7d63d83d485c5fb175a8f2972ac560841603542d3fb756cf6f45776328110",
    ("bi", ("big",), 12): "be2ae4b64bbe0fed68d94b7752de1a6701c9aae286bcf66dd2a9393e449e3e61",
    ("bi", ("angles",), 5): "ccf4af7a572ac6e8442f6377e522d935b697d3ed7fb4c8bb8048f14bb8147996",
    ("bi", ("angles",), 12): "330b13e92719d2bc55f408159232adcc9e4080ecade3e7de6f14151fa899b0b8",
    ("tr", (), 5): "07c341372abf18a277c0bb563c711b3c48d117a19f8e81d88ec66f36232d235e",
    ("tr", (), 12): "5f3a46542c9c7d74f0dd4a80e254d9a6ef6ec8e996e873e617e2eb7e1d898c73",
    ("tr", ("big",), 5): "f32a1eb8b40712ff2ce31d3d478fe791820186c2be33c9b7c48f2b6536975b2d",
    ("tr", ("big",), 12): "fffe24df66c224ce72d285ef2368a58f04c4c7fdce94c94a6e1e962bc82f43ea",
    ("tr", ("angles",), 5): "fea29b4b87c0cd76ef7069677b70ec5c093b03f33585fa8c1c32928cbf56a673",
    ("tr", ("angles",), 12): "72e897cb4b5cee5cdf2f0828e37c3a9e84248a55e577ebf1639202589b9da1f8",
    ("eval", (), 5): "00ce34d79eab9aecb26d352c4ba5c67438d855f065534a50d799c9a41509d216",
    ("eval", (), 12): "87079418db16864dc50ecfd2a4132997bcad67672ad734fea5b7ccf9f9c2c847",
    ("eval", ("big",), 5): "89f42448f98fa06ad39dad6b7b955f35c7e154b5050c4e2ce72d86c133f94e8c",
    ("eval", ("big",), 12): "6c9e922c1997e27c4721d5113cd0389b3648b1ad58a0b1d9d4473907d95b8922",
    ("eval", ("angles",), 5): "2b56acb9d57943e7dc8905fbadca3e7a5e11b2785db66801b173ae16a3bf4849",
    ("eval", ("angles",), 12): "bbcd51aee75078f947fe1600b68e137064fee1a94451aa03a9be38702468c63d",
}


@pytest.mark.parametrize("mode", ["bi", "tr", "eval"])
def test_the_older_modes_draw_what_they_drew(mode):
    for (m, flags, seed), digest in OLD_DRAWS.items():
        if m != mode:
            continue
        draws = fo.draw_cases(50, seed, mode, set(flags))
        got = hashlib.sha256("\n".join(fo.case_key(draws[c]) for c in range(50)).encode()).hexdigest()
        assert got == digest, (mode, flags, seed)


@pytest.mark.parametrize("flags,cases,seed", fo.AFFINE_SWEEPS, ids=[f[0] if f else "plain" for f, _, _ in fo.AFFINE_SWEEPS])
def test_committed_sweeps_reach_every_class(flags, cases, seed):
    """Every chunk class of the pixel loop with a full and a partial last chunk, lambda 0.7, perturbed intrinsics, each
    source-depth defect, a changed range, each batch size, with and without an exposure change.  `angles` draws its
    initial states from fuzz_draws.draw_angle instead of tests/edge_states.py; `big` has no `normal` size."""
    cov = fo.coverage(fo.draw_cases(cases, seed, "affine", set(flags)).values(), "affine")
    exempt = {"angles": {"init_edge"}, "big": {"size_normal"}}.get(flags[0] if flags else "", set())
    assert set(fo.CHUNK_CLASSES) | {"last_partial", "last_full", "lambda_0.7", "k_perturb", "exposure", "no_exposure",
                                    "range_changed", "init_edge", "size_small", "size_strip"} <= set(cov)
    for k, v in cov.items():
        assert v > 0 or k in exempt, (flags, k, cov)
    if "big" in flags:
        assert cov["size_big"] > 0


def test_affine_draws_differ_from_bi_only_where_they_should():
    """The fields `affine` shares with `bi` come from the same stream positions within a case (lam included, which the
    other modes force to 1); the new draws come last."""
    rs_a, rs_b = np.random.RandomState(3), np.random.RandomState(3)
    a, b = fo.draw_case(rs_a, "affine", set()), fo.draw_case(rs_b, "bi", set())
    for k in ("nl", "seed", "defect_seed", "holes", "k_perturb", "src_defects", "range", "upload_range", "max_iter", "lam",
              "init", "n_pairs"):
        assert a[k] == b[k], k
    assert a["tgt_defects"] == [] and "exposure" in a and "exposure" not in b


def test_the_checker_alone_stays_inside_the_caps_on_the_plain_sweep():
    flags, cases, seed = fo.AFFINE_SWEEPS[0]
    assert flags == ()
    from oracle import oracle
    oracle.build()
    draws = fo.draw_cases(cases, seed, "affine", set())
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ.setdefault(v, "1")
    with cf.ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1), mp_context=mp.get_context("spawn")) as pool:
        res = list(pool.map(fo.precheck_affine, draws.values(), chunksize=4))
    tally = collections.Counter()
    for r in res:
        tally.update({k: int(v) for k, v in r.items() if k != "bar"})
    tally["flat"] = tally["finite"] - tally["scaled"]
    print(dict(tally))
    assert tally["unstable"] <= 0.01 * cases, tally          # the 5 % cap cannot be filled by the inputs
    assert tally["flat"] >= 2 * cases / 3, tally
    levels = tally["by_threshold"] + tally["by_count"]
    assert tally["by_threshold"] >= 0.1 * levels and tally["by_count"] >= 0.1 * levels, tally
