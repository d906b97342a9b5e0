"""What tests/test_gpu_engine_history.py relies on, checked without a device (tests/engine_history.py):
  * every distinct case of every vocabulary step ends finite on the CPU checker of its objective, with cond <= 1e5 (the
    project's bar is then the flat 1e-9) and well-posed: one ulp of fx moves the checker's own result by less than a
    quarter of the bar (the guard of Expect and BiExpect);
  * the thresholded configuration stops cases by its thresholds on both levels, none near one; no decision of the
    trust-region checker is knife-edge;
  * the sequences are deterministic and contain what they promise, by the steps' labels (the GPU file asserts the same
    from the launch records it observes): every transition between users of the owner buffer at distance 1 and 2, the
    buffers that sit through non-users, growth and shrinkage under each objective, initial states and then none, a skipped
    level after all levels, pool B from larger and from smaller scratch; each random seed draws every user kind, a
    pipelined stretch, an evaluate call and a pool move.
A step that fails a guard gets other inputs, not a looser guard."""
import numpy as np
import pytest

import engine_history as eh

KEYS = eh.anchor_keys()


@pytest.mark.parametrize("key", list(KEYS), ids=[f"{s.name}-case{c}" for s, c in KEYS.values()])
def test_vocabulary_case_is_finite_flat_and_well_posed(key):
    step, case = KEYS[key]
    a = eh.anchor(step, case)
    assert a.finite, a.state
    assert a.flat, "cond above 1e5: the bar would not be the flat 1e-9"
    assert a.bar <= 1e-9 * max(1.0, float(np.abs(a.state).max()))
    sens, bar = a.guard()
    assert sens < 0.25 * bar, f"chaotic case: one ulp of fx moves the checker by {sens:.3e}, bar {bar:.1e}"
    if step.objective == "trust_region":
        assert a.margin > eh.gtr.MARGIN, a.margin
        assert all(r["noise_from"] is None for r in a.recs.values())
        assert sorted(a.recs) == [l for l in range(eh.NUM_LEVELS) if l not in step.skipped]


def test_every_step_has_its_anchors_and_its_labels():
    for step in eh.VOCABULARY.values():
        assert step.user in eh.USERS + ("none",)
        assert len(step.kinds) == sum(m > 0 for m in step.max_iter) + (step.user == "slide+fallback")
        assert all(eh.anchor_key(step, c) in KEYS for c in step.which)
        assert max(step.which) < (5 if step.pool == "A" else 3)
        src, tgt, init = eh.pair_list(step)
        assert len(src) == len(tgt) == len(step.which) and (init is None or init.shape == (len(src), 6))
        assert (init is not None) == (step.inits or max(step.which) >= 3)
    sizes = {len(s.which) for s in eh.VOCABULARY.values()}
    assert {1, 2, 8, 40, 48, 520} <= sizes
    assert 20 <= len(eh.VOCABULARY) <= 45


def test_thresholds_stop_cases_on_both_levels_and_none_is_near_one():
    step = eh.VOCABULARY["threshold40"]
    its, margin = [], np.inf
    for case in (0, 1, 2):
        a = eh.anchor(step, case)
        its.append(a.its)
        for level, g in a.e.gradient_norms:
            margin = min(margin, abs(g - step.min_grad[level]) / step.min_grad[level])
    its = np.array(its)
    assert np.all(its.min(axis=0) < np.array(step.max_iter)), its          # some case stops early on each level
    assert len({tuple(i) for i in its}) > 1, its                           # ... and not all alike: data-dependent counts
    assert margin > 0.05, margin


def test_large_rotation_cases_are_the_sliding_window_tests():
    """Cases 3 and 4 are the pair and the two initial states of test_sliding_window_hands_large_motions_to_the_exact_kernel."""
    big = eh.pool_problems("A")[3]
    assert np.allclose(big["motion"], eh.BIG_MOTION)
    assert abs(eh.case_init("A", 3, False)[3] - 0.30) < 0.01 and eh.case_init("A", 4, False)[3] == 0.17
    assert abs(eh.anchor(eh.VOCABULARY["slide48_handover"], 4).state[3] - 0.30) < 0.05      # it does converge outwards


def _labels(sequence):
    return [eh.VOCABULARY[n].user for n in eh.step_names(sequence)]


def test_scripted_sequence_contains_every_transition():
    names = eh.step_names(eh.SCRIPTED)
    users = _labels(eh.SCRIPTED)
    assert all(kind == "align" for kind, _ in eh.SCRIPTED)                 # serial: consecutive enqueues alternate slots
    missing = eh.required_transitions() - eh.transitions(users)
    assert not missing, sorted(missing)
    assert len(eh.required_transitions()) == 40
    assert eh.sits_through_non_users(users) == set(eh.TAGGERS)
    assert eh.growth_chains(names) == {"exact", "bi", "tr", "affine"}
    for prefix in ("exact", "bi", "tr", "affine"):                         # ... the 520-pair slot serves 2, later 520 again
        i = names.index(prefix + "520")
        assert names[i + 2] == prefix + "2" and names[i + 4] == prefix + "520"
    pairs2 = list(zip(names, names[2:]))
    assert ("exact40_init", "exact40") in pairs2
    assert ("tr40", "tr40_skip") in pairs2 and ("tr48", "tr40_skip") in pairs2
    steps = [eh.VOCABULARY[n] for n in names]
    moves = [(len(a.which), len(b.which)) for a, b in zip(steps, steps[1:]) if a.pool != b.pool]
    assert any(a > b for a, b in moves) and any(a < b for a, b in moves), moves
    assert {s.pool for s in steps} == {"A", "B"}
    assert any(3 in s.which for s in steps)                                # a hand-over to the exact kernel


def test_pipelined_stretches():
    for kind, names in eh.PIPELINED:
        assert kind == "pipe"
    first, second = (eh.step_names([item]) for item in eh.PIPELINED)
    after = {eh.VOCABULARY[b].user for a, b in zip(first, first[1:]) if a == "long40"}
    assert after == set(eh.USERS) | {"none"}
    assert {eh.VOCABULARY[a].user for a, b in zip(second, second[1:]) if b == "long40"} >= {"wide", "tr-HBM"}
    long40 = eh.VOCABULARY["long40"]
    assert long40.max_iter[0] > 1023 and len(long40.which) == 40
    # the short steps that can really overlap the long one share its configuration: no set_config in between
    for name in ("long_wide2", "long_tr2"):
        assert (eh.VOCABULARY[name].max_iter, eh.VOCABULARY[name].min_grad) == (long40.max_iter, long40.min_grad)


def test_evaluate_calls_move_the_watermark_both_ways():
    (l0, n0), (l1, n1), (l2, n2), (l3, n3), (l4, n4) = eh.EVAL_CALLS
    assert (l0, n0) == (1, 1) and l1 == 0 and (l2, n2) == (1, 3) and (l3, n3) == (0, 1)
    # the regrown workspace: as many owner entries as the call before it, more pairs
    assert eh.EVALUATE_REGROWN[:2] == [("eval", 3), ("eval", 4)] and l4 == 1 and n4 > n3
    for w, h in eh.POOLS.values():
        assert n4 * int(np.prod(eh.oracle.level_size(w, h, l4))) <= n3 * w * h
    for pool in eh.POOLS:
        assert n1 > eh.eval_group(pool, 0)                                 # more pairs than one 256 MB group holds
        src, tgt, states, level = eh.eval_arguments(pool, 1)
        assert len(src) == n1 and states.shape == (n1, 6) and max(tgt) < 6
    calls = [w for k, w in eh.WITH_EVALUATE if k == "eval"]
    assert set(calls) == {0, 1, 2, 3}
    assert [w for k, w in eh.WITH_EVALUATE if k == "eval"][:4] == [0, 1, 2, 3]
    inside = [n for k, w in eh.WITH_EVALUATE if k == "pipe" for n in w if n.startswith("eval:")]
    assert {int(n[5:]) for n in inside} == {0, 1, 2, 3}
    assert {eh.VOCABULARY[n].pool for n in eh.step_names(eh.WITH_EVALUATE)} == {"A", "B"}


@pytest.mark.parametrize("seed", eh.RANDOM_SEEDS)
def test_random_sequences_are_deterministic_and_draw_everything(seed):
    seq = eh.random_sequence(seed, eh.RANDOM_LENGTH)
    assert seq == eh.random_sequence(seed, eh.RANDOM_LENGTH) and len(seq) == eh.RANDOM_LENGTH
    assert seq != eh.random_sequence(seed + 1, eh.RANDOM_LENGTH)
    assert seq[:20] == eh.random_sequence(seed, 20)
    names = eh.step_names(seq)
    assert set(_labels(seq)) == set(eh.USERS) | {"none"}
    pools = [eh.VOCABULARY[n].pool for n in names]
    assert any(a != b for a, b in zip(pools, pools[1:]))
    kinds = {k for k, _ in seq}
    assert kinds == {"align", "pipe", "eval"}
    assert any(n.startswith("eval:") for k, w in seq if k == "pipe" for n in w)
    assert not any(n.startswith("long") for n in names)
