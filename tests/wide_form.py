"""Inputs that put the many-workgroup form of a Gauss-Newton level (csrc/gn_wide_kernels.hip) on its tile, stop and batch
edges, and what the oracle makes of them; shared by tests/test_wide_form_cpu.py (which vouches for them without a GPU) and
tests/test_gpu_wide_form.py (which runs them).  Test infrastructure, not collected as tests.  Nothing here touches a GPU:
the oracle alone (phovo_amd.native is imported for its constants).

The form restates the whole iteration instead of instantiating level_body: its own warp with a plain round(), its own rows,
tile sums in HBM that every tile workgroup adds again in 8 interleaved subsets (t = sub, sub + 8, ...), the solve and the
termination test at the head of the NEXT pass 1, the state in a two-slot buffer indexed by the iteration count's parity, and
a host loop that looks at the per-pair done words after iterations 4, 12, 20, ... while at least 4 iterations remain.

This module holds
  * the tiling and the host's look schedule restated (the library exposes neither);
  * sizes on every tile-count boundary of the interleaved sum, three pairs each, the last tile's depth all valid;
  * seeded initial states of one 82x100 pair, searched so that with a gradient threshold of 230 every stop count occurs, each
    gradient norm of each trace at least 1e-6 (relative) away from the threshold; batches chosen from them for every way
    the host loop can end; a two-level case that enters level 0 from either slot of the state buffer;
  * a pair without rows and sources with 3, 4, 5, 6 and 40 valid depths spread over the tiles;
  * the exact half-pixel problem and the narrow strips at this form's sizes;
  * the oracle's result of every case (Ref: counts, valid pixels, gradient norm, flags, the conditioned pose bar).
"""
import functools

import numpy as np

import extension_forms as ef
import plan_boundaries as pb

import phovo_amd  # noqa: F401
from phovo_amd import native, se3, synthetic
from oracle import oracle

# ------------------------------------------------------------------------------------------------------------------------
# the tiling and the host loop, restated (csrc/gn_wide_kernels.hip)
# ------------------------------------------------------------------------------------------------------------------------
WAVE = pb.WAVE
TILE_CHUNKS = 16          # :30   64-pixel chunks per tile
TILE_PX = TILE_CHUNKS * WAVE
SUM_SUBSETS = 8           # :64   SOLVE_T / NRED interleaved subsets of the tile sums
FIRST_LOOK, LOOK_EVERY, LOOK_RESERVE = 4, 8, 4            # gn_run_level_wide: next_check, its step, the iterations that must remain

POSE_TOL = pb.POSE_TOL
COND_MAX = pb.COND_MAX
GRAD_TOL = pb.GRAD_TOL
MARGIN = 1e-6             # decision margin: relative distance of every gradient norm from the threshold
MIN_DEPTH, MAX_DEPTH = 0.3, 5.0
NOWHERE = np.array([1e4, 0.0, 0.0, 0.0, 0.0, 0.0])       # ten kilometres to the side: no pixel lands in the target image


def tiles(n):
    return (n + TILE_PX - 1) // TILE_PX


def last_tile(n):
    """(first pixel, pixel count) of the last tile."""
    first = (tiles(n) - 1) * TILE_PX
    return first, n - first


def subset_sizes(n):
    """How many tile sums each of the 8 interleaved subsets adds."""
    return [len(range(s, tiles(n), SUM_SUBSETS)) for s in range(SUM_SUBSETS)]


def host_looks(max_iter, threshold):
    """The iteration counts after whose launch the host reads the done words: 4 + 8 j while max_iter - count >= 4, and
    none without a gradient threshold."""
    if not threshold > 0.0:
        return []
    return [c for c in range(FIRST_LOOK, max_iter + 1, LOOK_EVERY) if max_iter - c >= LOOK_RESERVE]


def launched_iterations(max_iter, threshold, stops):
    """Iterations the host launches for a batch whose pairs stop after `stops` iterations.  The step of iteration i is
    taken at the head of pass 1 of iteration i + 1, so a look after launching `c` iterations sees the stops up to c - 1."""
    for c in host_looks(max_iter, threshold):
        if all(s <= c - 1 for s in stops):
            return c
    return max_iter


def size_id(size):
    return f"{size[0]}x{size[1]}"


def cfgs(max_iter, min_grad=None):
    """(native, oracle) configuration: no blur, Scharr scale 1/16, lambda 1, depth range 0.3 ... 5."""
    return pb.cfgs(max_iter, min_grad)


def pyramids(p, ocfg):
    return pb._pyramids(ocfg, p)


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
class Ref(pb.PhotoRef):
    """pb.PhotoRef plus the project's conditioned pose bar (test_gpu_large_rotations.Expect: 1e-9 x max(1, cond / 1e5),
    capped at 1e-5; flat 1e-9 wherever cond(J^T J) <= 1e5), the flags the device reports for a finite run, and, per level,
    the iteration at which the state is not finite for the first time."""

    def __init__(self, ocfg, K, planes, init=None):
        super().__init__(ocfg, K, planes, None if init is None else np.asarray(init, dtype=np.float64))
        self.max_iter = [ocfg.max_num_iterations[l] for l in range(self.nl)]
        self.bar = min(1e-5, POSE_TOL * max(1.0, self.cond / COND_MAX))
        executed = [l for l in range(self.nl) if self.max_iter[l] > 0]
        self.flags = native.PAIR_RANK_DEFICIENT if any(self.valid[l] < 6 for l in executed) else 0
        self.first_nonfinite = [0] * self.nl
        for e in self.trace:
            if self.first_nonfinite[e["level"]] == 0 and not np.all(np.isfinite(e["state"])):
                self.first_nonfinite[e["level"]] = e["iteration"]

    def level_gnorms(self, level):
        return [g for l, g in self.gnorms if l == level]


def margin(ref, thresholds):
    """The smallest relative distance of a gradient norm of the trace from its level's threshold (inf without one)."""
    out = np.inf
    for l, g in ref.gnorms:
        if thresholds[l] > 0.0:
            out = min(out, abs(g - thresholds[l]) / thresholds[l])
    return out


# ------------------------------------------------------------------------------------------------------------------------
# 1. tile counts and partial tiles
# ------------------------------------------------------------------------------------------------------------------------
# (w, h): tiles, pixels in the last tile
TILE_SIZES = {
    (32, 32): (1, 1024),          # one full tile
    (33, 31): (1, 1023),          # last chunk of 63 lanes
    (41, 25): (2, 1),             # the second tile holds one pixel
    (112, 64): (7, 1024),         # one of the 8 sum subsets is empty
    (128, 64): (8, 1024),
    (82, 100): (9, 8),            # subset 0 adds two tiles
    (128, 128): (16, 1024),
    (129, 127): (16, 1023),
    (145, 113): (17, 1),
}
TILE_ITERS = 3
TILE_PAIRS = 3
# (seeds whose motion keeps the image's last pixel inside the image up to the last iteration: a one-pixel tile that is warped
# out of the image would count nothing)
TILE_SEEDS = (50, 52, 53)
# Where the last tile holds at least a chunk, losing it must move the oracle's pose by more than this.  The 1- and 8-pixel
# tiles end in the image's last pixels, whose Scharr gradient is exactly 0 under reflect-101 (the corner) or which carry too
# little weight: there the exact valid-pixel count is what tells a tile that was dropped.
TILE_POSE_MOVES = 1e-6


@functools.lru_cache(maxsize=None)
def tile_pairs(size):
    """Three pairs of `size` whose last tile has valid source depth at every pixel (holes there take the median depth)."""
    w, h = size
    out = []
    for i in range(TILE_PAIRS):
        p = dict(synthetic.make_pair(TILE_SEEDS[i], w, h, holes=0.02, trans=0.004 * (i + 1) * w / 640 + 0.002,
                                     rot=0.002 * (i + 1)))
        d = np.array(p["depth0"], dtype=np.float64)
        flat = d.reshape(-1)
        ok = (flat > MIN_DEPTH) & (flat < MAX_DEPTH)
        first, _ = last_tile(w * h)
        tail = flat[first:]
        tail[~ok[first:]] = np.median(flat[ok])
        p["depth0"] = d
        out.append(p)
    return out


def without_last_tile(p):
    """The pair with its last tile's source depth zeroed: what a sum that forgets the tile sees."""
    q = dict(p)
    d = p["depth0"].copy()
    first, _ = last_tile(d.size)
    d.reshape(-1)[first:] = 0.0
    q["depth0"] = d
    return q


@functools.lru_cache(maxsize=None)
def tile_ref(size, i, dropped=False):
    p = tile_pairs(size)[i]
    _, ocfg = cfgs([TILE_ITERS])
    return Ref(ocfg, p["K"], pyramids(without_last_tile(p) if dropped else p, ocfg))


# ------------------------------------------------------------------------------------------------------------------------
# 2. stop iteration, buffer parity, host looks
# ------------------------------------------------------------------------------------------------------------------------
STOP_SIZE = (82, 100)
STOP_SEED = 40
THRESHOLD = 230.0
N_CANDIDATES = 400
CANDIDATE_SEED = 2024
CANDIDATE_SCALE = np.array([0.01, 0.01, 0.01, 0.004, 0.004, 0.004])
LONG = 50                 # max_iter of the batches the host loop leaves early


@functools.lru_cache(maxsize=None)
def stop_pair(size=STOP_SIZE):
    w, h = size
    return synthetic.make_pair(STOP_SEED, w, h, holes=0.02, trans=0.004 * w / 640 + 0.002, rot=0.004)


@functools.lru_cache(maxsize=None)
def _stop_planes(size, nl):
    _, ocfg = cfgs([1] * nl)
    return pyramids(stop_pair(size), ocfg)


@functools.lru_cache(maxsize=None)
def stop_ref(init, max_iter, min_grad, size=STOP_SIZE):
    """The oracle on the stop pair from `init` (a tuple) under the given per-level limits (tuples)."""
    _, ocfg = cfgs(list(max_iter), list(min_grad))
    return Ref(ocfg, stop_pair(size)["K"], _stop_planes(size, len(max_iter)), np.array(init))


def stop_count(gnorms, max_iter, threshold=THRESHOLD):
    """Iterations a level runs given the gradient norm of each iteration: the update is applied, then the level is left if
    the count has reached max_iter or the norm is below the threshold."""
    for i, g in enumerate(gnorms[:max_iter]):
        if g < threshold:
            return i + 1
    return max_iter


@functools.lru_cache(maxsize=None)
def candidates():
    """Seeded random initial states around zero whose run of LONG iterations without a threshold is finite and keeps every
    gradient norm at least MARGIN (relative) from THRESHOLD: [(state tuple, gradient norm of each of the LONG iterations)].
    (The nearest-neighbour gradient norm is not monotone: the states are searched, not reasoned about.)"""
    rs = np.random.RandomState(CANDIDATE_SEED)
    out = []
    for _ in range(N_CANDIDATES):
        init = tuple(float(v) for v in rs.uniform(-1.0, 1.0, 6) * CANDIDATE_SCALE)
        r = stop_ref(init, (LONG,), (0.0,))
        g = r.level_gnorms(0)
        if r.finite and min(abs(x - THRESHOLD) for x in g) >= MARGIN * THRESHOLD:
            out.append((init, g))
    return out


def _first_with(counts_wanted, max_iter, taken, never=False):
    """The first candidate not yet taken that stops after one of `counts_wanted` iterations (never: without having met
    the threshold)."""
    for k, (init, g) in enumerate(candidates()):
        if k in taken or stop_count(g, max_iter) not in counts_wanted:
            continue
        if never and min(g[:max_iter]) < THRESHOLD:
            continue
        taken.add(k)
        return init
    raise AssertionError(("no candidate left", counts_wanted, max_iter, never))


@functools.lru_cache(maxsize=None)
def mixed_states(n=32):
    """The mixed batch: two states of every stop count 1 ... 16 under max_iter 16 -- one of the two with count 16 never meets
    the threshold --, shuffled; for n > 32 further candidates behind them."""
    taken = set()
    states = [_first_with({16}, 16, taken, never=True)]
    for c in list(range(1, 16)) + [16] + list(range(1, 16)):
        states.append(_first_with({c}, 16, taken))
    order = np.random.RandomState(5).permutation(len(states))
    states = [states[i] for i in order]
    while len(states) < n:
        states.append(_first_with(set(range(1, 17)), 16, taken))
    return tuple(states[:n])


@functools.lru_cache(maxsize=None)
def early_states(last, inner):
    """Eight states for max_iter LONG that all stop after at most `last` iterations, one of them after exactly `last`, one
    after 1 and at least one inside `inner` (a tuple of counts, may be empty)."""
    taken = set()
    states = [_first_with({last}, LONG, taken), _first_with({1}, LONG, taken)]
    if inner:
        states.append(_first_with(set(inner), LONG, taken))
    wanted = set(range(1, last + 1))
    while len(states) < 8:
        states.append(_first_with(wanted, LONG, taken))
    return tuple(states)


STOP_BATCHES = ("mixed16", "mixed13", "never_looks7", "one_look8", "leaves_first_look", "leaves_second_look", "no_threshold5")


def stop_batches():
    """name -> (max_iter, threshold, initial states)."""
    mixed = mixed_states()
    return {
        "mixed16": (16, THRESHOLD, mixed),                         # looks after 4 and 12, nobody leaves early
        "mixed13": (13, THRESHOLD, mixed),                         # odd final parity; one look (13 - 12 < 4)
        "never_looks7": (7, THRESHOLD, mixed),                     # 7 - 4 < 4
        "one_look8": (8, THRESHOLD, mixed),
        "leaves_first_look": (LONG, THRESHOLD, early_states(3, ())),
        "leaves_second_look": (LONG, THRESHOLD, early_states(11, (5, 6, 7, 8, 9, 10, 11))),
        "no_threshold5": (5, 0.0, mixed),
    }


EARLY_LEAVING = ("leaves_first_look", "leaves_second_look")


def batch_refs(name):
    max_iter, thr, states = stop_batches()[name]
    return [stop_ref(s, (max_iter,), (thr,)) for s in states]


# Two levels from 164x200, both in this form: level 1 is 82x100 (9 tiles), level 0 has 32 800 pixels, 33 tiles with 32 pixels
# in the last.  Level 0 starts from the slot of the state buffer that level 1's stop count selects.
TWO_SIZE = (164, 200)
TWO_MAX_ITER = (9, 9)
TWO_MIN_GRAD = (900.0, THRESHOLD)         # level 0, level 1 (the gradient norm grows with the pixel count)


@functools.lru_cache(maxsize=None)
def two_level_states():
    """Eight of the candidate states: four that leave level 1 of the 164x200 pair after an odd count, four after an even one,
    every gradient norm of both levels MARGIN from its threshold."""
    odd, even = [], []
    for init, _ in candidates():
        r = stop_ref(init, TWO_MAX_ITER, TWO_MIN_GRAD, TWO_SIZE)
        if not r.finite or margin(r, TWO_MIN_GRAD) < MARGIN:
            continue
        side = odd if r.its[1] % 2 else even
        if len(side) < 4:
            side.append(init)
        if len(odd) == len(even) == 4:
            break
    return tuple(v for pair in zip(odd, even) for v in pair)


def two_level_refs():
    return [stop_ref(s, TWO_MAX_ITER, TWO_MIN_GRAD, TWO_SIZE) for s in two_level_states()]


# ------------------------------------------------------------------------------------------------------------------------
# 3. position and batch size: the mixed batch, each pair alone, reversed, and with 40 pairs
# ------------------------------------------------------------------------------------------------------------------------
POSITION_SIZES = (32, 40)         # the automatic rule stops at 32 pairs; policy 1 takes any count


# ------------------------------------------------------------------------------------------------------------------------
# 4. no rows and too few rows
# ------------------------------------------------------------------------------------------------------------------------
BAD_SLOT = 4
NO_ROWS = {"one_level": (STOP_SIZE, (3,)), "two_levels": (TWO_SIZE, (3, 3))}


def no_rows_states():
    """Eight initial states of the stop pair: the first eight candidates."""
    return [c[0] for c in candidates()[:8]]


@functools.lru_cache(maxsize=None)
def no_rows_ref(name, slot):
    """The oracle for a slot of the batch; slot BAD_SLOT starts at NOWHERE."""
    size, max_iter = NO_ROWS[name]
    init = tuple(NOWHERE) if slot == BAD_SLOT else no_rows_states()[slot]
    return stop_ref(init, max_iter, (0.0,) * len(max_iter), size)


FEW_ROWS = (3, 4, 5, 6, 40)
FEW_ITERS = 3
FEW_COPIES = 9


@functools.lru_cache(maxsize=None)
def few_rows_pixels(n_valid):
    """Linear indices of the only pixels with valid source depth: one in the last tile (of 8 pixels), the others seeded, in
    tiles of their own as long as there are tiles (40: spread over all nine), away from the borders."""
    w, h = STOP_SIZE
    n = w * h
    first, count = last_tile(n)
    rs = np.random.RandomState(n_valid)
    px = [first + count // 2]
    tile_order = [t % (tiles(n) - 1) for t in range(n_valid - 1)]
    while len(px) < n_valid:
        t = tile_order[len(px) - 1]
        k = int(rs.randint(t * TILE_PX, (t + 1) * TILE_PX))
        r, c = divmod(k, w)
        if 10 <= c < w - 10 and 10 <= r < h - 10 and k not in px:
            px.append(k)
    return tuple(sorted(px))


@functools.lru_cache(maxsize=None)
def few_rows_pair(n_valid):
    w, h = STOP_SIZE
    p = dict(synthetic.make_pair(350, w, h))
    d = np.zeros(w * h)
    px = np.array(few_rows_pixels(n_valid))
    d[px] = p["depth0"].reshape(-1)[px]
    p["depth0"] = d.reshape(h, w)
    return p


@functools.lru_cache(maxsize=None)
def few_rows_ref(n_valid):
    p = few_rows_pair(n_valid)
    _, ocfg = cfgs([FEW_ITERS])
    return Ref(ocfg, p["K"], pyramids(p, ocfg))


def wild(v):
    """Metres / radians that are no alignment (tests/test_gpu_round3.py)."""
    return (not np.all(np.isfinite(v))) or np.max(np.abs(v)) > 10.0


# ------------------------------------------------------------------------------------------------------------------------
# 5. exact half-pixel projections
# ------------------------------------------------------------------------------------------------------------------------
HALF_SIZES = ((64, 48), (82, 100))        # 3 tiles; 9 tiles with 8 pixels in the last
HALF_PAIRS = (1, 9)
HALF_CELLS = [(size, sign, n) for size in HALF_SIZES for sign in (1.0, -1.0) for n in HALF_PAIRS]


@functools.lru_cache(maxsize=None)
def half_pixel(size, sign):
    """synthetic.half_pixel_problem with the target's gradients: (K, planes as five one-level lists, initial state, Ref)."""
    w, h = size
    K, i0, d0, i1, state = synthetic.half_pixel_problem(w, h, sign)
    gx, gy = oracle.scharr(i1, 0.0625)
    planes = [[i0], [d0], [i1], [gx], [gy]]
    _, ocfg = cfgs([1])
    return K, planes, state, Ref(ocfg, K, planes, state)


def half_pixel_targets(size, sign):
    """Projected (column, row) of every source pixel of the half-pixel problem at its initial state, in fp64 in the
    reference's operation order."""
    w, h = size
    K, planes, state, _ = half_pixel(size, sign)
    cc, rr = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    pz = planes[1][0]
    px = (cc - K[0, 2]) * pz * (1.0 / K[0, 0])
    py = (rr - K[1, 2]) * pz * (1.0 / K[1, 1])
    X, Y, Z = px + state[0], py + state[1], pz + state[2]
    return (X * K[0, 0]) * (1.0 / Z) + K[0, 2], (Y * K[1, 1]) * (1.0 / Z) + K[1, 2]


# ------------------------------------------------------------------------------------------------------------------------
# 6. narrow strips
# ------------------------------------------------------------------------------------------------------------------------
STRIP_ITERS = 3
STRIP_MIN_FINITE = 8


@functools.lru_cache(maxsize=None)
def strip_case(size):
    """(pair, its three initial states, fp64 planes) of a strip of ef.STRIPS."""
    p, states = ef.strip_cases(*size)
    _, ocfg = ef.configs([STRIP_ITERS])
    return p, states, ef.emulated_planes(ocfg, p, native.STORAGE_F64)


def strip_trace_loses_state(ocfg, K, planes, init):
    """Whether the oracle's trace has an iteration whose state is not finite (what ef.check_strip follows)."""
    _, _, tr = oracle.optimize(ocfg, K, *planes, init_state=init, want_trace=True)
    return any(not np.all(np.isfinite(t["state"])) for t in tr)
