"""Randomised sweep of the Gaussian pose prior of the two inverse-compositional objectives on the device
(gn_inverse_prior_kernel.hip, phovo_engine_enqueue_align_prior): the 150 cases of
tests/inverse_prior_sweep.py under both objectives, in chunks of 25.  Per pair the reference is the checker
(tests/inverse_prior_ref.py) on the device's own planes: iterations, rows, flags and (objective 6) outliers exact, delta to
4 ulp, the pose to inverse_ref.pose_bar(cond, state), gradient_norm to 1e-9 relative, error and prior_cost under
test_gpu_inverse_prior._compare's bars.  A pair with Lambda = 0, or with every level's scale 0, also has the bits of
align_pairs without a prior -- which ties the two kernels without a prior into the sweep.  A pair is set aside on the
checker's evidence alone (inverse_prior_sweep.set_aside), at most 5 % of them."""
import collections

import pytest

import phovo_amd  # noqa: F401

import inverse_prior_sweep as sw
from test_gpu_inverse_prior import IDS, OBJECTIVES, ROBUST, _align, _compare, _device_pyramid, _engine, _kinds, _record, _upload

pytestmark = pytest.mark.gpu

_tally = {}


def _run_chunk(c, objective):
    """(pairs compared or set aside, Counter of the reasons, worst distance / bar) of chunk c, run once."""
    if (c, objective) in _tally:
        return _tally[(c, objective)]
    robust = objective == ROBUST
    total, reasons, worst, plain_pairs = 0, collections.Counter(), 0.0, 0
    for i in range(c * sw.CHUNK, (c + 1) * sw.CHUNK):
        d = sw.problem(i)
        n, nl = d["n"], d["nl"]
        with _engine(objective, d["K"], d["w"], d["h"], 2, d["mi"], d["mg"], d["lam"], d["scales"]) as eng:
            _upload(eng, [d["p"]])
            pyr = _device_pyramid(eng, 0, 1, nl, d["mi"])
            s, reps, preps, rob = _align(eng, objective, [0] * n, [1] * n, d["priors"], d["Lambdas"], d["inits"])
            assert [l["levels"] for l in eng.last_launches()] == [[l] for l in range(nl - 1, -1, -1)]
            bare = [k for k in range(n) if sw.no_prior(d, k)]
            if bare:
                ps, preps_plain = eng.align_pairs([0] * len(bare), [1] * len(bare), init_states=d["inits"][bare],
                                                  want_reports=True)
                _kinds(eng, objective, prior=False)
                prob = eng.fetch_robust_reports(len(bare)) if robust else [None] * len(bare)
        for j, k in enumerate(bare):
            got = _record(s[k], reps[k], None, None if rob is None else rob[k], nl)
            assert got == _record(ps[j], preps_plain[j], None, prob[j], nl), (i, k)
            if d["classes"][k] == "zero":
                assert preps["prior_cost"][k] == 0.0
            plain_pairs += 1
        for k in range(n):
            ref = sw.reference(d, pyr, k, robust)
            total += 1
            why = sw.set_aside(ref, robust)
            if why:
                reasons[why] += 1
                print(f"case {i} pair {k} set aside: {why}")
                continue
            print(f"case {i} ({d['w']}x{d['h']}, {nl} levels, scales {d['scales']}) pair {k} ({d['classes'][k]}):")
            worst = max(worst, _compare(s[k], reps[k], preps[k], None if rob is None else rob[k], ref, d["Lambdas"][k], nl,
                                        margins=False))
    _tally[(c, objective)] = (total, reasons, worst, plain_pairs)
    return _tally[(c, objective)]


@pytest.mark.parametrize("objective", OBJECTIVES, ids=IDS)
@pytest.mark.parametrize("c", range(sw.CHUNKS))
def test_sweep_chunk(c, objective):
    total, reasons, worst, plain_pairs = _run_chunk(c, objective)
    aside = sum(reasons.values())
    print(f"chunk {c}: {total} pairs, {aside} set aside {dict(reasons)}, {plain_pairs} also held to the call without a prior, "
          f"worst distance / bar {worst:.3g}")
    assert aside <= sw.SET_ASIDE_CAP * total


def test_sweep_set_aside_share():
    total, reasons, worst, plain_pairs = 0, collections.Counter(), 0.0, 0
    for objective in OBJECTIVES:
        for c in range(sw.CHUNKS):
            t, r, w, p = _run_chunk(c, objective)
            total, worst, plain_pairs = total + t, max(worst, w), plain_pairs + p
            reasons.update(r)
    aside = sum(reasons.values())
    print(f"sweep: {total} pairs, set aside {aside} ({100.0 * aside / total:.2f} %) {dict(reasons)}; {plain_pairs} pairs also "
          f"held bit for bit to the call without a prior; worst distance / bar {worst:.3g}")
    assert aside <= sw.SET_ASIDE_CAP * total and plain_pairs >= 100
