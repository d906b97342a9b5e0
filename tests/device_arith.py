"""Inputs and exact references for the device arithmetic helpers of csrc/gn_device.hpp (fast_rcp, round_half_up_from, the
index maps, mad24_uniform_b, plane_load, the three solvers).  Test infrastructure, not collected as tests: shared by
tests/test_device_arith_cpu.py (no GPU: the references and the inputs themselves), tests/test_gpu_device_arith.py (the
helpers on the device, through tests/native/arith_probe.hip) and tests/test_oracle_properties.py (the rounding table).

Everything is drawn from fixed seeds and computed once per process (functools.lru_cache); callers do not modify what
they get.
"""
import functools
import math
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS53 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------------
# round_half_up_from
# ------------------------------------------------------------------------------------------------------------------------
def exact_round(v):
    """C round() -- half away from zero -- of the double v, in rational arithmetic (integers)."""
    p, q = float(v).as_integer_ratio()                      # v = p / q exactly
    return (2 * p + q) // (2 * q) if p >= 0 else -((-2 * p + q) // (2 * q))


@functools.lru_cache(maxsize=None)
def round_candidates():
    """Every neighbour (six doubles either side) of every tie, integer and quarter point up to image sizes and beyond,
    400 000 random values and the edges of the admitted range (the helper's contract covers v > -0.5; the table holds a
    few values at and below that bound too, which the callers filter)."""
    cands = []
    for n in list(range(0, 70)) + [127, 128, 255, 256, 511, 512, 1023, 1024, 1279, 1280, 2047, 2048, 65535, 65536, 2 ** 20, 2 ** 30]:
        for base in (n, n + 0.25, n + 0.5, n + 0.75, n + 1.0):
            for k in range(-6, 7):
                y = np.float64(base)
                for _ in range(abs(k)):
                    y = np.nextafter(y, np.inf if k > 0 else -np.inf)
                cands.append(float(y))
    rng = np.random.RandomState(0)
    cands += list(rng.uniform(-0.5, 2000.0, 200000)) + list(rng.uniform(-0.5, 1.5, 200000))
    cands += [float(np.nextafter(-0.5, 0.0)), -0.25, -1e-300, 0.0, 5e-324]
    return tuple(cands)


@functools.lru_cache(maxsize=None)
def round_table():
    """(v, exact round of v) for the candidates with v > -0.5, as float64 arrays (every rounded value is far below 2^53)."""
    v = np.array([c for c in round_candidates() if c > -0.5], dtype=np.float64)
    return v, np.array([float(exact_round(x)) for x in v], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# fast_rcp
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rcp_inputs():
    """dict name -> float64 array, all finite with 2^-1000 <= |x| <= 2^1000 (+ a little: the pattern points sit on the
    bounds' inside)."""
    rng = np.random.default_rng(4801)
    wide = np.ldexp(rng.uniform(1.0, 2.0, 500000), rng.integers(-1000, 1000, 500000)) * np.where(rng.random(500000) < 0.5, -1.0, 1.0)
    depth = rng.uniform(0.05, 50.0, 100000)
    pat = []
    for k in range(-1000, 1001, 37):
        p = math.ldexp(1.0, k)
        pat += [p, float(np.nextafter(p, np.inf)), float(np.nextafter(p, 0.0)), 3.0 * p,
                math.ldexp(float(np.nextafter(2.0, 0.0)), k)]
    pat = [x for x in pat if 2.0 ** -1000 <= x <= 2.0 ** 1000]
    pat = np.array(pat + [-x for x in pat])
    near_one = [1.0]
    up = down = 1.0
    for _ in range(64):
        up, down = float(np.nextafter(up, np.inf)), float(np.nextafter(down, 0.0))
        near_one += [up, down]
    near_one = np.array(near_one + [-x for x in near_one])
    return dict(wide=wide, depth=depth, patterns=pat, near_one=near_one)


def ulp_distance(a, b):
    """Number of doubles between a and b (finite, same sign, neither zero nor subnormal): difference of the bit patterns."""
    ia = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(ia - ib)


def rcp_relative_error(x, r):
    """|r - 1/x| / |1/x| = |r x - 1| of two doubles, exactly (a Fraction)."""
    return abs(Fraction(float(r)) * Fraction(float(x)) - 1)


# ------------------------------------------------------------------------------------------------------------------------
# rowcol_from_index, rowcol_from_index_floor, rowcol_advance
# ------------------------------------------------------------------------------------------------------------------------
ROWCOL_WIDTHS = tuple(range(1, 701)) + (1023, 1024, 1025, 1279, 1280, 1919, 1920, 2047, 2048, 4095, 4096)
MAX_PIXELS = 1 << 21
NEGATIVE_WIDTHS = tuple(range(1, 41)) + (53, 80, 160, 333, 640) + ROWCOL_WIDTHS[700:]       # floor form, k in [-4096, 0)


@functools.lru_cache(maxsize=None)
def rowcol_boundary_points():
    """(W[], k[]) int64: for every width of ROWCOL_WIDTHS the pixels either side of a row boundary, k = rW - 1, rW, rW + 1
    with 0 <= k < 2^21, for the first 40 rows, the middle row and the last two rows of the tallest image of that width
    (H = 2^21 // W; r = H, the first row past it, is included for its k = HW - 1, the last pixel)."""
    ws, ks = [], []
    for W in ROWCOL_WIDTHS:
        H = MAX_PIXELS // W
        rows = sorted(set(r for r in list(range(0, 40)) + [H // 2, H - 2, H - 1, H] if 0 <= r <= H))
        k = sorted(set(r * W + d for r in rows for d in (-1, 0, 1) if 0 <= r * W + d < MAX_PIXELS))
        ws += [W] * len(k)
        ks += k
    return np.array(ws, dtype=np.int64), np.array(ks, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def rowcol_random_points():
    """2e5 random (W, k): 3125 widths (log-uniform in 1 .. 4096) with 64 pixels each, 0 <= k < min(2^21, a tall image)."""
    rng = np.random.default_rng(733)
    W = np.floor(2.0 ** rng.uniform(0.0, 12.0, 3125)).astype(np.int64).clip(1, 4096)
    W = np.repeat(W, 64)
    k = rng.integers(0, MAX_PIXELS, W.size)
    return W, k


@functools.lru_cache(maxsize=None)
def rowcol_negative_points():
    """(W[], k[]) for the floor form: every k in [-4096, 0) for the widths of NEGATIVE_WIDTHS."""
    W = np.repeat(np.array(NEGATIVE_WIDTHS, dtype=np.int64), 4096)
    k = np.tile(np.arange(-4096, 0, dtype=np.int64), len(NEGATIVE_WIDTHS))
    return W, k


def fma_exact(a, b, c):
    """The correctly rounded a * b + c of three doubles (int / int division of a Fraction rounds to nearest even)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def rowcol_emulated(k, W, floor_form):
    """The helper's own arithmetic with IEEE operations: (column, row) as Python floats."""
    w = float(W)
    inv_w = 1.0 / w
    half_inv_w = 0.5 * inv_w
    q = fma_exact(float(k), inv_w, half_inv_w)
    rd = float(math.floor(q)) if floor_form else float(math.trunc(q))
    cd = fma_exact(-rd, w, float(k))
    return cd, rd


WALK_THREADS = (64, 256, 512, 1024)
WALK_WIDTHS = (5, 40, 53, 80, 160, 333, 640, 1280)


@functools.lru_cache(maxsize=None)
def rowcol_walks():
    """The chunk walk of a whole level of n = W * (2^21 // W) pixels for every workgroup size and width, first and last
    lane: dict of int arrays W, start, step_r, step_c, steps, threads.  A lane starts at its own index and advances by
    `threads` pixels per call: step_r = threads // W, step_c = threads % W (< W: the single-wrap precondition)."""
    rows = []
    for threads in WALK_THREADS:
        for W in WALK_WIDTHS:
            n = W * (MAX_PIXELS // W)
            for start in (0, threads - 1):
                rows.append((W, start, threads // W, threads % W, (n - 1 - start) // threads, threads))
    a = np.array(rows, dtype=np.int64)
    return dict(W=a[:, 0], start=a[:, 1], step_r=a[:, 2], step_c=a[:, 3], steps=a[:, 4], threads=a[:, 5])


# ------------------------------------------------------------------------------------------------------------------------
# mad24_uniform_b
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mad24_cases():
    """list of (b, a[], c[], note): every a * b + c below 2^31.  b is one value per launch (a scalar register)."""
    rng = np.random.default_rng(2404)
    top = 1 << 21
    out = []
    # corners of [0, 2^21]^3 that keep the result below 2^31
    for b in (0, 1, 2, 1023, 1024, top - 1, top):
        amax = top if b == 0 else min(top, ((1 << 31) - 1 - top) // b)
        a = np.array([0, 1, amax // 2, max(amax - 1, 0), amax], dtype=np.int64)
        c = np.array([0, 1, top // 2, top - 1, top], dtype=np.int64)
        A, C = np.meshgrid(a, c, indexing="ij")
        out.append((b, A.reshape(-1), C.reshape(-1), "corners"))
    # 1e5 random values: 100 widths b, 1000 (a, c) each
    for _ in range(100):
        b = int(rng.integers(0, top + 1))
        amax = top if b == 0 else min(top, ((1 << 31) - 1 - top) // b)
        out.append((b, rng.integers(0, amax + 1, 1000), rng.integers(0, top + 1, 1000), "random"))
    # the kernels' domain at its edges: a = row < H, b = W, c = column < W, H * W <= 2^21
    for W in (1, 2, 5, 40, 53, 640, 1280, 2048, 4096, top // 2, top):
        H = top // W
        a = np.array(sorted(v for v in set([0, 1, H // 2, H - 2, H - 1]) if 0 <= v < H), dtype=np.int64)
        c = np.array(sorted(v for v in set([0, 1, W // 2, W - 2, W - 1]) if 0 <= v < W), dtype=np.int64)
        A, C = np.meshgrid(a, c, indexing="ij")
        out.append((W, A.reshape(-1), C.reshape(-1), "domain"))
    # the limits of the instruction's 24-bit signed operands, where it is still exact: a = 2^23 - 1 and a = -1
    out.append((255, np.array([(1 << 23) - 1] * 2, dtype=np.int64), np.array([0, 12345], dtype=np.int64), "a = 2^23 - 1"))
    out.append((4096, np.array([-1] * 2, dtype=np.int64), np.array([4096, 5000], dtype=np.int64), "a = -1"))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# plane_load
# ------------------------------------------------------------------------------------------------------------------------
STORAGE = {0: np.float64, 1: np.float32, 2: np.float16}


@functools.lru_cache(maxsize=None)
def load_plane(storage):
    """A plane of the storage type holding +-0, subnormals (every fp16 one; 1e4 of fp32 and of fp64), the smallest normal,
    the largest finite value, +-inf, NaN and ordinary values."""
    t = STORAGE[storage]
    rng = np.random.default_rng(90 + storage)
    fi = np.finfo(t)
    special = [0.0, -0.0, fi.tiny, -fi.tiny, fi.max, -fi.max, np.inf, -np.inf, np.nan, 1.0, -1.5, 0.1]
    if storage == 2:
        sub = np.arange(1, 1 << 10, dtype=np.uint16).view(np.float16)
    elif storage == 1:
        sub = rng.integers(1, 1 << 23, 10000).astype(np.uint32).view(np.float32)
    else:
        sub = rng.integers(1, 1 << 52, 10000).astype(np.uint64).view(np.float64)
    sub = np.concatenate([sub, -sub])
    plain = rng.uniform(-255.0, 255.0, 3000).astype(t)
    return np.concatenate([np.array(special, dtype=t), sub, plain]).astype(t)


# ------------------------------------------------------------------------------------------------------------------------
# the solvers
# ------------------------------------------------------------------------------------------------------------------------
PER_COND = 40
# Worst error of the REFERENCE's method (inverse by partially pivoted LU, then a product: reference_lu_inverse_solve below)
# on the random draws, as a multiple of cond2(H) * 2^-53 * |x_exact|; tests/test_device_arith_cpu.py recomputes both from
# the seed.  The solvers' bar is four times that: two backward-stable algorithms round differently.
REFERENCE_FACTOR = {6: 1.555, 8: 1.869}
MARGIN = 4.0


def bar_factor(n):
    return MARGIN * REFERENCE_FACTOR[n]


def upper(H):
    """The upper triangle of a symmetric matrix, row-major (tri / tri8 of gn_device.hpp)."""
    H = np.asarray(H)
    return H[np.triu_indices(H.shape[0])].copy()


def full(h, n):
    """The symmetric matrix of an upper triangle (what the solvers see: they never read below the diagonal)."""
    H = np.zeros((n, n), dtype=np.asarray(h).dtype)
    H[np.triu_indices(n)] = h
    return H + np.triu(H, 1).T


CONDS_LOG10 = tuple(range(0, 15, 2))
CONDS = tuple(float(10 ** e) for e in CONDS_LOG10)          # 1, 1e2, ..., 1e14


@functools.lru_cache(maxsize=None)
def random_spd(n):
    """320 draws Q diag(s) Q^T: cond 1 .. 1e14 in steps of 100, 40 per step, overall scale 1e-3 .. 1e6.  Returns
    (h [N, n (n + 1) / 2], g [N, n], nominal cond [N]).
    The draws are the same bits on every machine: nothing goes through LAPACK, BLAS or the maths library (the worst error
    of a solver over 320 systems moves by a third when the systems change in their last bits).  Q is a product of n
    Householder reflections of uniform random vectors, s are powers of ten with exponents spread evenly between 0 and
    -log10(cond) (rounded to integers, shuffled), the scale is a uniform mantissa times a power of ten, and every sum is
    a Python loop over IEEE doubles."""
    rng = np.random.default_rng(6800 + n)
    hs, gs, cs = [], [], []
    for e10, cond in zip(CONDS_LOG10, CONDS):
        for _ in range(PER_COND):
            Q = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
            for v in rng.uniform(-1.0, 1.0, size=(n, n)).tolist():
                vv = 0.0
                for a in v:
                    vv += a * a
                for row in Q:
                    t = 0.0
                    for a, b in zip(row, v):
                        t += a * b
                    t = 2.0 * t / vv
                    for j in range(n):
                        row[j] -= t * v[j]
            expo = [int(round(e10 * i / (n - 1.0))) for i in rng.permutation(n).tolist()]
            k10 = int(rng.integers(-3, 6))
            scale = float(rng.uniform(1.0, 10.0)) * (float(10 ** k10) if k10 >= 0 else 1.0 / float(10 ** -k10))
            s = [scale / float(10 ** e) for e in expo]
            H = np.zeros((n, n))
            for i in range(n):
                for j in range(i, n):
                    t = 0.0
                    for k in range(n):
                        t += Q[i][k] * s[k] * Q[j][k]
                    H[i, j] = H[j, i] = t
            hs.append(upper(H))
            gs.append(rng.uniform(-1.0, 1.0, size=n) * scale)
            cs.append(cond)
    return np.array(hs), np.array(gs), np.array(cs)


@functools.lru_cache(maxsize=None)
def real_systems():
    """The badly scaled systems of real alignments: dict(n6=(h, g), n8=(h, g), chol=(a, b)), from the four committed
    golden cases at the first and last iteration of each level:
      n6    the numpy twin's H, g (recorded in the fixtures by tests/golden/make_golden.py);
      n8    tests/affine_ref.py's system along its own level loop;
      chol  the Levenberg-Marquardt system (S H S + clamp(diag) / radius) y = S g that tests/trust_region_ref.py forms."""
    import phovo_amd  # noqa: F401
    from oracle import numpy_twin as twin
    import affine_ref
    import trust_region_ref as trr
    n6, n8, chol = [], [], []
    for name in "abcd":
        z = np.load(os.path.join(HERE, "golden", f"case_{name}.npz"))
        nl = int(z["num_levels"])
        lev = z["exp_trace_level"]
        for L in sorted(set(lev.tolist())):
            idx = np.flatnonzero(lev == L)
            for i in sorted({int(idx[0]), int(idx[-1])}):
                n6.append((upper(z["exp_trace_hessian"][i]), z["exp_trace_gradient"][i].copy()))
        K = z["K"]
        pyr = twin.build_pyramids(z["gray0"], z["depth0"], z["gray1"], nl, [float(v) for v in z["grad_scale"]])
        lo, hi = float(z["min_depth"]), float(z["max_depth"])
        # the affine checker's level loop (affine_ref.optimize), keeping the systems
        state = np.concatenate([z["init_state"], [0.0, 0.0]])
        for L in range(nl - 1, -1, -1):
            kept = []
            for it in range(int(z["max_iter"][L])):
                g, H, _ = affine_ref.system(pyr[L], L, K, state, lo, hi)
                kept.append((upper(H), g.copy()))
                state = state - float(z["lam"][L]) * np.linalg.solve(H, g)
                if np.linalg.norm(g) < float(z["min_grad"][L]):
                    break
            n8 += kept[:1] + kept[-1:] if len(kept) > 1 else kept
        # the trust-region checker, Ceres's default options; the first system is damped by the initial radius at the
        # level's first evaluation, the last one by the final radius at the final point
        x = np.array(z["init_state"], dtype=np.float64)
        opts = dict(function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_radius=1e4,
                    max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3)
        for L in range(nl - 1, -1, -1):
            mi = int(z["max_iter"][L])
            if mi <= 0:
                continue
            i0, d0, i1, gx, gy = pyr[L]
            first = []

            def evaluate_at(s):
                ev = trr.evaluate(i0, d0, i1, gx, gy, L, K, s, lo, hi)
                if not first:
                    first.append(ev)
                return ev
            x, rec = trr.optimize_level(evaluate_at, x, mi, **opts)
            for H, g, radius in ((first[0]["H"], first[0]["g"], opts["initial_radius"]), (rec["H"], rec["g"], rec["final_radius"])):
                S = rec["S"]
                Hs = S[:, None] * H * S[None, :]
                A = Hs + np.diag(np.clip(np.diag(Hs), 1e-6, 1e32) / radius)
                chol.append((upper(A), S * g))

    def pack(rows):
        return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    return dict(n6=pack(n6), n8=pack(n8), chol=pack(chol))


def solver_systems(kind):
    """(h, g) of every finite, non-singular system a solver is held to: kind 'n6' (solve6_ldlt), 'n8' (solve8_ldlt),
    'chol' (solve6_cholesky, on the 6 x 6 draws); the random draws first, then the real ones."""
    n = 8 if kind == "n8" else 6
    h, g, _ = random_spd(n)
    rh, rg = real_systems()[kind]
    return np.concatenate([h, rh]), np.concatenate([g, rg])


def _exact(h, g, n):
    import mpmath
    xs, conds = [], []
    with mpmath.workprec(400):
        for hh, gg in zip(h, g):
            H = full(hh, n)
            # what mpmath.lu_solve runs (LU_decomp, L_solve, U_solve), with the factorisation kept for the inverse
            LU, p = mpmath.mp.LU_decomp(mpmath.matrix(H.tolist()))
            solve = lambda b: mpmath.mp.U_solve(LU, mpmath.mp.L_solve(LU, b, p))
            xs.append([float(v) for v in solve(mpmath.matrix(gg.tolist()))])
            inv64 = np.array([[float(v) for v in solve(mpmath.mp.unitvector(n, j + 1))] for j in range(n)]).T
            conds.append(np.linalg.norm(H, 2) * np.linalg.norm(inv64, 2))
    return np.array(xs), np.array(conds)


@functools.lru_cache(maxsize=None)
def _exact_random(n):
    h, g, _ = random_spd(n)
    return _exact(h, g, n)


@functools.lru_cache(maxsize=None)
def exact_solutions(kind):
    """(x_exact [N, n] rounded to fp64, cond2 [N]) of solver_systems(kind): mpmath's LU solve at 400 bits;
    cond2 = |H|_2 |H^-1|_2 with the inverse from the same factorisation (its fp64 rounding is entrywise good to 2^-53, so
    its norm is)."""
    n = 8 if kind == "n8" else 6
    xr, cr = _exact_random(n)
    rh, rg = real_systems()[kind]
    xe, ce = _exact(rh, rg, n)
    return np.concatenate([xr, xe]), np.concatenate([cr, ce])


def error_fraction(x, kind):
    """|x - x_exact|_2 / (cond2 * 2^-53 * |x_exact|_2) per system (x: the first len(x) systems of solver_systems(kind)):
    the bar is bar_factor(n)."""
    xe, cond = exact_solutions(kind)
    xe, cond = xe[:len(x)], cond[:len(x)]
    return np.linalg.norm(np.asarray(x) - xe, axis=1) / (cond * EPS53 * np.linalg.norm(xe, axis=1))


def reference_lu_inverse_solve(H, g):
    """The reference's own method as oracle/phovo_oracle.c restates it (inverse6): the inverse column by column from a
    partially pivoted LU, then inverse times g; plain IEEE doubles, any size."""
    n = len(g)
    lu = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    perm = list(range(n))
    for kc in range(n):
        piv = max(range(kc, n), key=lambda r: (abs(lu[r][kc]), -r))
        if piv != kc:
            lu[kc], lu[piv] = lu[piv], lu[kc]
            perm[kc], perm[piv] = perm[piv], perm[kc]
        d = lu[kc][kc]
        for r in range(kc + 1, n):
            lu[r][kc] /= d
            f = lu[r][kc]
            for c in range(kc + 1, n):
                lu[r][c] -= f * lu[kc][c]
    inv = [[0.0] * n for _ in range(n)]
    for col in range(n):
        y = [0.0] * n
        for r in range(n):
            s = 1.0 if perm[r] == col else 0.0
            for c in range(r):
                s -= lu[r][c] * y[c]
            y[r] = s
        for r in range(n - 1, -1, -1):
            s = y[r]
            for c in range(r + 1, n):
                s -= lu[r][c] * inv[c][col]
            inv[r][col] = s / lu[r][r]
    out = []
    for a in range(n):
        s = 0.0
        for b in range(n):
            s += inv[a][b] * float(g[b])
        out.append(s)
    return np.array(out)


def ldlt_numpy(h, g, n):
    """solve6_ldlt / solve8_ldlt restated in numpy over a batch (plain products and sums instead of fma): x [N, n]."""
    H = np.stack([full(hh, n) for hh in h]).astype(np.float64)
    N = H.shape[0]
    L = np.zeros((N, n, n)); Ld = np.zeros((N, n, n)); inv = np.zeros((N, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = H[:, j, j].copy()
            for k in range(j):
                dj = dj - L[:, j, k] * Ld[:, j, k]
            inv[:, j] = 1.0 / dj
            for i in range(j + 1, n):
                t = H[:, j, i].copy()
                for k in range(j):
                    t = t - L[:, i, k] * Ld[:, j, k]
                Ld[:, i, j] = t
                L[:, i, j] = t * inv[:, j]
        y = np.zeros((N, n)); x = np.zeros((N, n))
        for i in range(n):
            t = np.asarray(g, dtype=np.float64)[:, i].copy()
            for k in range(i):
                t = t - L[:, i, k] * y[:, k]
            y[:, i] = t
        for i in range(n - 1, -1, -1):
            t = y[:, i] * inv[:, i]
            for k in range(i + 1, n):
                t = t - L[:, k, i] * x[:, k]
            x[:, i] = t
    return x


def cholesky_numpy(a, b):
    """solve6_cholesky restated in numpy over a batch: (y [N, 6], ok [N])."""
    n = 6
    A = np.stack([np.triu(full(aa, n)) for aa in a]).astype(np.float64)      # A[:, k, j], k <= j: becomes L^T
    N = A.shape[0]
    ok = np.ones(N, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[:, j, j].copy()
            for k in range(j):
                d = d - A[:, k, j] * A[:, k, j]
            ok &= (d > 0.0) & (np.abs(d) <= np.finfo(np.float64).max)
            ljj = np.sqrt(d)
            A[:, j, j] = ljj
            for i in range(j + 1, n):
                t = A[:, j, i].copy()
                for k in range(j):
                    t = t - A[:, k, i] * A[:, k, j]
                A[:, j, i] = t / ljj
        z = np.zeros((N, n)); y = np.zeros((N, n))
        for i in range(n):
            t = np.asarray(b, dtype=np.float64)[:, i].copy()
            for k in range(i):
                t = t - A[:, k, i] * z[:, k]
            z[:, i] = t / A[:, i, i]
        for i in range(n - 1, -1, -1):
            t = z[:, i].copy()
            for k in range(i + 1, n):
                t = t - A[:, i, k] * y[:, k]
            y[:, i] = t / A[:, i, i]
    return y, ok


@functools.lru_cache(maxsize=None)
def singular_systems(n):
    """Exactly singular positive semi-definite systems J^T J of rank n - 1 with small-integer J, built so that the zero
    pivot is EXACT in the unpivoted factorisations: columns p and p + 1 of J are equal with a squared norm of 4 or 16, and
    the p columns in front of them are 2 e_k on rows of their own, so every quantity up to pivot p + 1 is a small integer
    or a power of two and d_{p+1} = h_pp - (h_pp / h_pp) h_pp = 0 without rounding.  One system per p = 0 .. n - 2 and per
    norm.  Returns (h, g, J list)."""
    rng = np.random.default_rng(5100 + n)
    hs, gs, Js = [], [], []
    for p in range(n - 1):
        for unit in (1, 2):
            m = p + 4 + 12
            J = np.zeros((m, n), dtype=np.int64)
            for k in range(p):
                J[k, k] = 2
            col = np.zeros(m, dtype=np.int64)
            col[p:p + 4] = unit * rng.choice([-1, 1], 4)             # squared norm 4 or 16
            J[:, p] = col
            J[:, p + 1] = col
            J[p:, p + 2:] = rng.integers(-3, 4, size=(m - p, n - p - 2))
            H = J.T @ J
            assert np.linalg.matrix_rank(H.astype(np.float64)) == n - 1, (n, p, unit)
            hs.append(upper(H.astype(np.float64)))
            gs.append((J.T @ rng.integers(-3, 4, m)).astype(np.float64))
            Js.append(J)
    return np.array(hs), np.array(gs), Js
