"""Extensions that are NOT in the reference (BASELINE.json configs[4]: Huber weights, narrow plane storage):
CPU-side checks -- the oracle's Huber IRLS against the independent numpy twin, and the optional yml keys."""
import os

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, se3, synthetic
from oracle import oracle, numpy_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config_files")


def _problem():
    p = synthetic.make_pair(17, 96, 72, holes=0.03)
    # a few gross outliers in the target, the thing robust weights are for
    g1 = p["gray1"].copy()
    g1[10:20, 30:44] = 255
    return p, g1


def test_oracle_huber_matches_twin():
    p, g1 = _problem()
    nl, max_iter, delta = 3, [2, 4, 6], [0.02, 0.05, 0.05]
    ocfg = oracle.make_config(num_levels=nl, max_iter=max_iter, min_grad=[0.0] * nl)
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(g1, ocfg)
    s1, it1, tr1 = oracle.optimize(ocfg, p["K"], i0p, d0p, i1p, gxp, gyp, want_trace=True, huber_delta=delta)
    pyr = twin.build_pyramids(p["gray0"], p["depth0"], g1, nl, [0.0625] * nl)
    s2, it2, tr2 = twin.optimize(pyr, p["K"], dict(num_levels=nl, lam=[1.0] * nl, max_iter=max_iter,
                                                    min_grad=[0.0] * nl, huber_delta=delta))
    assert it1 == it2 and len(tr1) == len(tr2)
    for a, b in zip(tr1, tr2):
        np.testing.assert_allclose(a["gradient"], b["gradient"], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(a["hessian"], b["hessian"], rtol=1e-9, atol=1e-9)
    assert se3.state_distance(s1, s2) < 1e-9
    # the weights do something: the plain least-squares result differs
    s0, _ = oracle.optimize(ocfg, p["K"], i0p, d0p, i1p, gxp, gyp)
    assert se3.state_distance(s0, s1) > 1e-5


def test_huber_off_and_huge_delta_equal_the_reference_path():
    p, g1 = _problem()
    nl = 3
    ocfg = oracle.make_config(num_levels=nl, max_iter=[2, 3, 4], min_grad=[0.0] * nl)
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(g1, ocfg)
    s0, it0 = oracle.optimize(ocfg, p["K"], i0p, d0p, i1p, gxp, gyp)
    s1, it1 = oracle.optimize(ocfg, p["K"], i0p, d0p, i1p, gxp, gyp, huber_delta=[0.0, -1.0, 0.0])
    s2, it2 = oracle.optimize(ocfg, p["K"], i0p, d0p, i1p, gxp, gyp, huber_delta=[1e9] * nl)
    assert it0 == it1 == it2
    assert np.array_equal(s0, s1) and np.array_equal(s0, s2)


def test_extension_keys_are_optional_in_the_yml(tmp_path):
    for name in sorted(os.listdir(CFG)):                       # the reference's files: everything off
        ext = native.read_extensions_file(os.path.join(CFG, name))
        assert ext.plane_storage == native.STORAGE_F64
        assert all(v == 0.0 for v in ext.huber_delta)
    base = open(os.path.join(CFG, "config_6_level_optimization_analytic.yml")).read()
    p = tmp_path / "config_6_level_huber_fp16.yml"
    p.write_text(base + "huber_delta (at each level): [0.1, 0.1, 0.05, 0.05, 0.05, 0.05]\nplane_storage_bits: 16\n")
    cfg = native.read_config_file(str(p))                       # the reference keys still parse
    assert cfg.num_levels == 6 and list(cfg.max_num_iterations[:6]) == [0, 0, 5, 20, 50, 50]
    ext = native.read_extensions_file(str(p))
    assert ext.plane_storage == native.STORAGE_F16
    assert list(ext.huber_delta[:6]) == [0.1, 0.1, 0.05, 0.05, 0.05, 0.05]
    bad = tmp_path / "bad.yml"
    bad.write_text(base + "plane_storage_bits: 8\n")
    with pytest.raises(native.PhovoError) as ei:
        native.read_extensions_file(str(bad))
    assert ei.value.status == 2


@pytest.mark.parametrize("corrected", [False, True])
def test_oracle_bilinear_matches_twin(corrected):
    """Bilinear forward-additive mode: the oracle (reference temps, optional `+x` slip) against the twin, which
    builds the Jacobian from the rotated point's derivatives instead -- two derivations, one answer."""
    p = synthetic.make_pair(31, 96, 72, holes=0.03)
    nl, mi = 3, [3, 5, 8]
    ocfg = oracle.make_config(num_levels=nl, max_iter=mi, min_grad=[0.0] * nl)
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    pyr = twin.build_pyramids(p["gray0"], p["depth0"], p["gray1"], nl, [0.0625] * nl)
    s1, it1, tr1 = oracle.optimize(ocfg, p["K"], i0p, d0p, i1p, gxp, gyp, want_trace=True,
                                   bilinear=True, corrected=corrected, huber_delta=[0.0, 0.03, 0.03])
    s2, it2, tr2 = twin.optimize(pyr, p["K"], dict(num_levels=nl, lam=[1.0] * nl, max_iter=mi, min_grad=[0.0] * nl,
                                                    bilinear=True, corrected=corrected, huber_delta=[0.0, 0.03, 0.03]))
    assert it1 == it2
    for a, b in zip(tr1, tr2):
        np.testing.assert_allclose(a["gradient"], b["gradient"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(a["hessian"], b["hessian"], rtol=1e-9, atol=1e-8)
    assert se3.state_distance(s1, s2) < 1e-9
    # and it is the better estimator on this synthetic pair than the reference's nearest/scatter formulation
    s0, _ = oracle.optimize(ocfg, p["K"], i0p, d0p, i1p, gxp, gyp)
    assert se3.state_distance(s1, p["motion"]) < se3.state_distance(s0, p["motion"])


def test_sampling_keys_in_yml(tmp_path):
    base = open(os.path.join(CFG, "config_4_level_optimization_analytic.yml")).read()
    p = tmp_path / "b.yml"
    p.write_text(base + "sampling_bilinear: 1\njacobian_corrected: 1\n")
    ext = native.read_extensions_file(str(p))
    assert ext.sampling == native.SAMPLING_BILINEAR and ext.jacobian_corrected == 1
    bad = tmp_path / "bad2.yml"
    bad.write_text(base + "sampling_bilinear: 2\n")
    with pytest.raises(native.PhovoError):
        native.read_extensions_file(str(bad))


# ---- CPU pre-checks of every deterministic input of tests/test_gpu_extension_forms.py (tests/extension_forms.py) ---------
import extension_forms as ef  # noqa: E402


def _vouch(ocfg, K, planes, init, huber, what, **ext):
    """Finite, well-posed for the pose bar (Expect's guard asserts it) and, with Huber weights, residuals beyond delta and a
    result away from the unweighted one."""
    e = ef.expect(ocfg, K, planes, init, huber, **ext)
    assert e.finite, what
    if huber is not None:
        assert ef.huber_bites(ocfg, K, planes, init, huber) > 0.005, what
        plain = ef.expect(ocfg, K, planes, init, None, **ext)
        assert se3.state_distance(e.state, plain.state) > 1e-6, what
    return e


@pytest.mark.parametrize("name", list(ef.FORMS))
def test_inputs_of_the_form_matrix_are_finite_well_posed_and_weighted(name):
    f = ef.FORMS[name]
    _, ocfg = ef.configs(f["max_iter"], f["min_grad"])
    pairs = ef.form_pairs(name)
    for st in f["settings"].get("storages", ef.STORAGES):
        for hub in (False, True):
            huber = ef.huber_deltas(f["max_iter"], hub)
            for k, (p, init) in enumerate(pairs):
                planes = ef.emulated_planes(ocfg, p, st, patched=(k == 0))
                if k == 0 and st == native.STORAGE_F16:          # the patches did put fp16 subnormals into every plane
                    l = max(l for l in range(len(f["max_iter"])) if f["max_iter"][l] > 0)
                    assert all(ef.count_f16_subnormals(planes[j][l]) >= 8 for j in (0, 2, 3, 4)), name
                _vouch(ocfg, p["K"], planes, init, huber, (name, st, hub, k))


@pytest.mark.parametrize("size,max_iter", ef.BILINEAR_SIZES, ids=[f"{s[0]}x{s[1]}" for s, _ in ef.BILINEAR_SIZES])
def test_inputs_of_the_bilinear_cells_are_finite_well_posed_and_weighted(size, max_iter):
    _, ocfg = ef.configs(max_iter)
    for st, corrected, hub in ef.bilinear_cells():
        huber = ef.huber_deltas(max_iter, hub)
        for k, (p, init) in enumerate(ef.bilinear_pairs(size)):
            planes = ef.emulated_planes(ocfg, p, st)
            _vouch(ocfg, p["K"], planes, init, huber, (size, st, corrected, hub, k), bilinear=True, corrected=corrected)


def test_inputs_of_the_narrow_storage_edges():
    # depth gate: the planted depths are inside the gate in fp64 and on it in fp32; the oracle counts exactly them
    K, planes, planted = ef.depth_gate_problem()
    _, ocfg = ef.configs([1], min_depth=ef.GATE[0], max_depth=ef.GATE[1])
    assert planted > 100
    e64 = _vouch(ocfg, K, planes, np.zeros(6), None, "gate f64")
    for st in ef.STORAGES:
        rounded = [[ef.round_depth(a[0], st) if j == 1 else ef.round_image(a[0], st)] for j, a in enumerate(planes)]
        e = _vouch(ocfg, K, rounded, np.zeros(6), None, ("gate", st))
        assert e64.valid[0] - e.valid[0] == planted, (e64.valid, e.valid, planted)
    # strips: at most half of the cases may be non-finite on the oracle; the finite ones pass the guard
    cases = bad = 0
    for w, h in ef.STRIPS:
        p, states = ef.strip_cases(w, h)
        _, ocfg = ef.configs([3])
        for st in ef.STORAGES:
            planes = ef.emulated_planes(ocfg, p, st)
            for hub in (False, True):
                for init in states:
                    e = ef.expect(ocfg, p["K"], planes, init, ef.huber_deltas([3], hub))
                    cases += 1
                    bad += not e.finite
    assert cases == 72 and 2 * bad <= cases, (bad, cases)
    # one-column / one-row bilinear levels on fp64 planes: finite on the oracle, which never reads the target's depth
    for (w, h), K, planes, depth1 in ef.one_column_problem():
        _, ocfg = ef.configs([2])
        assert np.isnan(depth1.reshape(-1)[0]) and np.isnan(depth1.reshape(-1)[1])
        e = _vouch(ocfg, K, planes, np.zeros(6), None, (w, h), bilinear=True, corrected=True)
        assert e.valid[0] >= 38, (w, h, e.valid)
    # fp16 overflow: a block of inf in the target's intensity leaves the oracle non-finite (the planted inf case)
    pairs = ef.form_pairs("threads256_80x60")
    _, ocfg = ef.configs([4])
    planes = ef.emulated_planes(ocfg, pairs[1][0], native.STORAGE_F16)
    planes[2][0][20:30, 30:50] = np.inf
    es, _ = oracle.optimize(ocfg, pairs[1][0]["K"], *planes)
    assert not np.all(np.isfinite(es))
    # the state-change test's pair under bilinear sampling
    _vouch(ocfg, pairs[0][0]["K"], ef.emulated_planes(ocfg, pairs[0][0], native.STORAGE_F16), np.zeros(6), None, "toggle",
           bilinear=True)
