"""The references and inputs of tests/test_gpu_device_arith.py, checked without a GPU (tests/device_arith.py):

* the index map of csrc/gn_device.hpp (rowcol_from_index, rowcol_from_index_floor), emulated with correctly rounded fma in
  rational arithmetic, equals integer divmod on every boundary point -- the header's claim holds in IEEE arithmetic, so a
  mismatch on the device would be the device's arithmetic;
* the solvers' bar: the reference's own method (inverse by partially pivoted LU, then a product) on the committed draws
  gives the factor the bar is four times of, and a plain numpy restatement of each solver stays inside the bar;
* every input set holds what it is there for: subnormals, ties, row boundaries, the condition numbers actually drawn.
"""
import math

import numpy as np
import pytest

import device_arith as da


def test_rowcol_emulation_is_divmod_on_every_boundary_point():
    W, k = da.rowcol_boundary_points()
    assert W.size > 85000 and set(W.tolist()) == set(da.ROWCOL_WIDTHS)
    wrong = 0
    for w, kk in zip(W.tolist(), k.tolist()):
        r, c = divmod(kk, w)
        for floor_form in (False, True):
            wrong += da.rowcol_emulated(kk, w, floor_form) != (float(c), float(r))
    assert wrong == 0


def test_rowcol_floor_emulation_is_floor_divmod_in_front_of_the_image():
    # (a sample of the device test's negative set: every k for three widths, every width for the k next to a boundary)
    W, k = da.rowcol_negative_points()
    keep = np.isin(W, (1, 53, 4096)) | (np.abs(k % W) <= 1) | (k % W == W - 1)
    assert keep.sum() > 20000
    for w, kk in zip(W[keep].tolist(), k[keep].tolist()):
        r, c = divmod(kk, w)                                  # Python: floor division, 0 <= c < w
        assert r < 0 and da.rowcol_emulated(kk, w, True) == (float(c), float(r)), (w, kk)
    # trunc is not floor there: the plain form is for k >= 0 only
    assert da.rowcol_emulated(-1, 5, False)[1] == 0.0 and da.rowcol_emulated(-1, 5, True) == (4.0, -1.0)


def test_rowcol_inputs_reach_the_boundaries():
    W, k = da.rowcol_boundary_points()
    assert np.all((k >= 0) & (k < da.MAX_PIXELS))
    c = k % W
    assert np.count_nonzero(c == 0) > 25000 and np.count_nonzero(c == W - 1) > 25000
    assert np.count_nonzero(k > da.MAX_PIXELS - 4200) > 700           # the last rows of the tallest images
    Wr, kr = da.rowcol_random_points()
    assert Wr.size == 200000 and Wr.min() == 1 and Wr.max() > 4000 and len(set(Wr.tolist())) > 1000
    assert np.all((Wr.reshape(-1, 64) == Wr.reshape(-1, 64)[:, :1]))  # one width per 64-thread workgroup
    Wn, kn = da.rowcol_negative_points()
    assert kn.min() == -4096 and kn.max() == -1 and Wn.size == 4096 * len(da.NEGATIVE_WIDTHS) <= 1000000


def test_walks_cover_a_whole_level_and_keep_the_single_wrap_precondition():
    w = da.rowcol_walks()
    assert len(w["W"]) == len(da.WALK_THREADS) * len(da.WALK_WIDTHS) * 2
    assert np.all(w["step_c"] < w["W"]) and np.all(w["step_c"] >= 0)                  # the helper's precondition
    assert np.all(w["step_r"] * w["W"] + w["step_c"] == w["threads"])
    assert np.any((w["W"] < w["threads"]) & (w["step_r"] > 0)) and np.any(w["step_r"] == 0)
    n = w["W"] * (da.MAX_PIXELS // w["W"])
    last = w["start"] + w["steps"] * w["threads"]
    assert np.all(last < n) and np.all(last + w["threads"] >= n) and np.all(n <= da.MAX_PIXELS)
    assert w["steps"].sum() <= 1000000
    # wraps happen, and steps without a wrap too, in the widths below the workgroup size
    i = int(np.flatnonzero((w["W"] == 53) & (w["threads"] == 64))[0])
    cols = (w["start"][i] + np.arange(1, 200) * 64) % 53
    assert np.any(np.diff(cols) < 0) and np.any(np.diff(cols) > 0)


def test_round_table_holds_ties_their_neighbours_and_the_edges():
    v, expect = da.round_table()
    assert v.size > 400000 and np.all(v > -0.5)
    frac = v - np.floor(v)
    assert np.count_nonzero(frac == 0.5) >= 80                            # ties
    below = np.nextafter(np.floor(v) + 0.5, -np.inf)
    assert np.count_nonzero(v == below) >= 80                             # the largest double below a tie
    assert np.nextafter(0.5, 0.0) in v and 0.0 in v and 5e-324 in v and np.count_nonzero(v < 0) > 50
    # the table's expectation is C round(): numpy's emulation of the two instructions agrees on all of it
    p = np.nextafter(0.5, 0.0)
    assert np.array_equal(np.floor(v + p), expect)
    assert np.count_nonzero(np.floor(v + 0.5) != expect) >= 1              # and the obvious form does not


def test_rcp_inputs():
    x = da.rcp_inputs()
    assert x["wide"].size == 500000 and x["depth"].size == 100000
    for name, a in x.items():
        assert np.all(np.isfinite(a)) and np.all(np.abs(a) >= 2.0 ** -1000) and np.all(np.abs(a) <= 2.0 ** 1000), name
    e = np.frexp(x["wide"])[1]
    assert e.min() < -990 and e.max() > 990 and np.count_nonzero(x["wide"] < 0) > 200000
    assert x["depth"].min() >= 0.05 and x["depth"].max() <= 50.0
    m = np.frexp(np.abs(x["patterns"]))[0]
    assert np.count_nonzero(m == 0.5) >= 100 and np.count_nonzero(m == 0.75) >= 100          # 2^k and 3 2^k
    assert np.count_nonzero(m == np.nextafter(1.0, 0.0)) >= 100 and np.count_nonzero(m == np.nextafter(0.5, 1.0)) >= 100
    assert 1.0 in x["near_one"] and np.nextafter(1.0, 2.0) in x["near_one"] and np.nextafter(1.0, 0.0) in x["near_one"]
    # the error measures: one ulp off is one ulp off, and the relative error of a correctly rounded quotient is < 2^-53
    assert da.ulp_distance(np.array([1.0]), np.array([np.nextafter(1.0, 2.0)]))[0] == 1
    assert da.rcp_relative_error(3.0, 1.0 / 3.0) < 2.0 ** -53 and da.rcp_relative_error(3.0, 0.3333) > 1e-5


def test_mad24_cases_stay_in_range_and_reach_the_edges():
    top = 1 << 21
    n_random, notes = 0, set()
    for b, a, c, note in da.mad24_cases():
        notes.add(note)
        r = a * b + c
        assert np.all(r < 2 ** 31) and np.all(r >= -(2 ** 31)), note
        assert -(1 << 23) <= b < (1 << 23) and np.all(a >= -(1 << 23)) and np.all(a < (1 << 23)), note
        if note in ("corners", "random", "domain"):
            assert 0 <= b <= top and np.all((a >= 0) & (a <= top) & (c >= 0) & (c <= top))
        if note == "random":
            n_random += a.size
        if note == "domain":
            H = top // b
            assert a.max() == H - 1 and c.max() == b - 1 and r.max() == H * b - 1 <= top - 1
    assert n_random == 100000 and notes == {"corners", "random", "domain", "a = 2^23 - 1", "a = -1"}
    assert any(note == "domain" and (a * b + c).max() == top - 1 for b, a, c, note in da.mad24_cases())


def test_load_planes_hold_subnormals_and_specials():
    for storage, t in da.STORAGE.items():
        p = da.load_plane(storage)
        assert p.dtype == t
        fi = np.finfo(t)
        sub = np.isfinite(p) & (p != 0) & (np.abs(p) < fi.tiny)
        assert np.count_nonzero(sub) >= (2046 if storage == 2 else 20000), storage
        assert np.count_nonzero(np.isnan(p)) == 1 and np.count_nonzero(np.isinf(p)) == 2
        assert fi.max in p and -fi.max in p and fi.tiny in p
        assert np.count_nonzero((p == 0) & np.signbit(p)) == 1 and np.count_nonzero((p == 0) & ~np.signbit(p)) == 1
        wide = p.astype(np.float64)                           # widening is exact: narrowing it again gives the same bits
        assert np.array_equal(wide.astype(t).view(np.uint8), p.view(np.uint8)) or np.isnan(p).any()
        ok = ~np.isnan(p)
        assert np.array_equal(wide[ok].astype(t), p[ok])
    assert np.count_nonzero(np.isin(np.arange(1, 1024, dtype=np.uint16).view(np.float16), da.load_plane(2))) == 1023


@pytest.mark.parametrize("n", [6, 8])
def test_random_draws_span_the_condition_numbers(n):
    h, g, nominal = da.random_spd(n)
    assert h.shape == (len(da.CONDS) * da.PER_COND, n * (n + 1) // 2) and g.shape == (h.shape[0], n)
    kind = "n6" if n == 6 else "n8"
    _, cond = da.exact_solutions(kind)
    cond = cond[:h.shape[0]]
    for c in da.CONDS:                                        # the drawn condition number is the nominal one (to rounding)
        sel = nominal == c
        assert sel.sum() == da.PER_COND
        assert np.all(np.abs(cond[sel] / c - 1.0) < max(1e-12, 20.0 * c * da.EPS53)), c      # (H is rounded: cond moves by ~cond eps)
    norms = np.array([np.linalg.norm(da.full(hh, n), 2) for hh in h])
    assert norms.min() < 1e-2 and norms.max() > 1e5                         # the overall scale
    for hh in h[::37]:
        assert np.all(np.linalg.eigvalsh(da.full(hh, n)) > 0)


def test_real_systems_are_there_and_badly_scaled():
    real = da.real_systems()
    for kind, n in (("n6", 6), ("n8", 8), ("chol", 6)):
        h, g = real[kind]
        assert h.shape[0] >= 16 and h.shape[1] == n * (n + 1) // 2 and g.shape == (h.shape[0], n), kind
        assert np.all(np.isfinite(h)) and np.all(np.isfinite(g))
        nrand = da.random_spd(n)[0].shape[0]
        cond = da.exact_solutions(kind)[1][nrand:]
        diag = np.array([np.diag(da.full(hh, n)) for hh in h])
        print(kind, "systems", h.shape[0], "cond2 %.3g .. %.3g" % (cond.min(), cond.max()),
              "diagonal ratio up to %.3g" % (diag.max(1) / diag.min(1)).max())
        # (the Levenberg-Marquardt system is Jacobi-scaled: its diagonal is level by construction)
        assert np.all(diag > 0) and cond.max() > 100.0 and (kind == "chol" or (diag.max(1) / diag.min(1)).max() > 5.0), kind


@pytest.mark.parametrize("kind", ["n6", "n8"])
def test_reference_method_gives_the_factor_the_bar_is_built_on(kind):
    """c = 4 x the worst error of the reference's own method on the random draws, in units of cond2 2^-53 |x|: recomputed
    here from the seed and compared with the committed figure, so that the bar cannot move unnoticed.  (The draws and the
    method are loops over IEEE doubles, the same bits everywhere; 1e-3 covers the four digits the figure is written with.)"""
    n = 6 if kind == "n6" else 8
    h, g, _ = da.random_spd(n)
    x = np.array([da.reference_lu_inverse_solve(da.full(hh, n), gg) for hh, gg in zip(h, g)])
    frac = da.error_fraction(x, kind)
    worst = float(frac.max())
    print(kind, "reference method: worst factor %.4f at draw %d, bar factor c = %.3f" % (worst, int(frac.argmax()), da.bar_factor(n)))
    assert abs(worst / da.REFERENCE_FACTOR[n] - 1.0) < 1e-3, worst
    assert da.bar_factor(n) == 4.0 * da.REFERENCE_FACTOR[n]
    # the restatement solves: against numpy's own solver on a well-conditioned draw
    np.testing.assert_allclose(x[0], np.linalg.solve(da.full(h[0], n), g[0]), rtol=1e-12)


@pytest.mark.parametrize("kind", ["n6", "n8", "chol"])
def test_numpy_restatement_of_each_solver_is_inside_the_bar(kind):
    n = 8 if kind == "n8" else 6
    h, g = da.solver_systems(kind)
    if kind == "chol":
        x, ok = da.cholesky_numpy(h, g)
        assert ok.all()
    else:
        x = da.ldlt_numpy(h, g, n)
    frac = da.error_fraction(x, kind)
    print(kind, "numpy restatement: worst fraction of the bar %.3f" % (frac.max() / da.bar_factor(n)))
    assert np.all(frac <= da.bar_factor(n)), (int(frac.argmax()), frac.max())


@pytest.mark.parametrize("n", [6, 8])
def test_singular_systems_have_an_exact_zero_pivot(n):
    h, g, Js = da.singular_systems(n)
    assert h.shape[0] == 2 * (n - 1)
    from fractions import Fraction
    for hh, J in zip(h, Js):
        H = da.full(hh, n)
        assert np.array_equal(H, (J.T @ J).astype(np.float64)) and np.abs(H).max() < 2 ** 20      # small integers: exact
        # rank n - 1 in rational arithmetic: unpivoted elimination meets exactly one zero pivot, with a zero column under it
        M = [[Fraction(int(v)) for v in row] for row in H]
        zero = 0
        for j in range(n):
            if M[j][j] == 0:
                zero += 1
                assert all(M[i][j] == 0 for i in range(j, n))
                continue
            for i in range(j + 1, n):
                f = M[i][j] / M[j][j]
                M[i] = [a - f * b for a, b in zip(M[i], M[j])]
        assert zero == 1
    x = da.ldlt_numpy(h, g, n)
    assert np.all(~np.isfinite(x).all(axis=1))                             # the restated LDL^T: a non-finite component each
    if n == 6:
        assert not da.cholesky_numpy(h, g)[1].any()


def test_cholesky_restatement_rejects_what_the_device_must_reject():
    h, g, _ = da.random_spd(6)
    H = da.full(h[3], 6)
    bad = []
    neg = H.copy(); neg[2, 2] = -neg[2, 2]; bad.append(neg)
    nan = H.copy(); nan[0, 3] = nan[3, 0] = math.nan; bad.append(nan)
    for j in range(6):
        inf = H.copy(); inf[j, j] = math.inf; bad.append(inf)
    _, ok = da.cholesky_numpy(np.array([da.upper(b) for b in bad]), np.tile(g[3], (len(bad), 1)))
    assert not ok.any()
