"""What the level kernels' pixel loops keep around their arithmetic, on every launch form (run with -m gpu on an MI355X).

Pass 2 of level_body (csrc/gn_kernels.hip) forms the residual of a pixel nobody landed on as a plain difference of two
loads that the frame descriptor's range check answers with 0 -- the I1 load of such a lane gets bit 31 of its owner entry,
-1, into its byte offset -- and with the owner map in LDS the entries of the map, the running pixel counter of both passes
and the owner slot read a chunk ahead are byte offsets of the intensity plane, not indices.  Nothing of that takes part in
the arithmetic, so every case here has the bars of tests/test_gpu_twist_row.py (poses within POSE_TOL of the oracle,
iteration counts and valid pixels equal, gradient norm within GRAD_TOL, the well-posedness of every reference) and passes
on a build without these forms as well:

* ownerless rows: rendered pairs of seed 140 under a motion along the optical axis, three fixed iterations from near the
  truth.  Backwards (z = -0.35) the ownerless rows lie among the owned ones, forwards (z = +0.35) whole border rows, the
  first and the last chunk included, are ownerless; at least a quarter of the Jacobian rows at the true motion are
  (asserted on the CPU).  One wave, 256, 512 and 1024 threads, the fused launch, the owner map in HBM, and fp32 / fp16
  planes at 256 threads;
* every pixel its own owner: source and target are the same frame, the state is zero, one iteration -- every residual is
  I(k) - I(k), so the gradient norm is exactly 0.0 and the state stays exactly zero; an owner entry off by one element or
  one shift shows at once.  The last size of every form with the map in LDS (the largest byte offset, 38 783 * 8), in
  fp64, fp32 and fp16;
* more than 32 chunks per wave: the last size at which no wave carries more than 32 chunks and the first at which one
  carries 33, at 256 threads, 1024 threads and in the fused launch, and one size with a partial last chunk each; holes of
  0.03, so that the ballots differ from chunk to chunk.
"""
import functools

import numpy as np
import pytest

import edge_states
import plan_boundaries as pb

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, se3, synthetic
from oracle import numpy_twin, oracle

POSE_TOL, GRAD_TOL = pb.POSE_TOL, pb.GRAD_TOL
ITERS = 3
SEED = 140
CAP_THRESHOLD = 1e-3              # a threshold (the fused launch needs one) that no gradient norm comes near: the cap ends the level
FUSED_COPIES = 9
PAIRS = 2
STORAGES = {"f64": native.STORAGE_F64, "f32": native.STORAGE_F32, "f16": native.STORAGE_F16}


def _pyramids(ocfg, p):
    i0p, d0p = oracle.build_source_pyramids(p["gray0"], p["depth0"], ocfg)
    i1p, gxp, gyp = oracle.build_target_pyramids(p["gray1"], ocfg)
    return i0p, d0p, i1p, gxp, gyp


def _planes(ocfg, p, storage):
    return _pyramids(ocfg, p) if storage == native.STORAGE_F64 else pb.storage_planes(ocfg, p, storage)


def well_posed(ref):
    assert ref.finite and ref.cond < pb.COND_MAX, ref.cond
    moved, its = ref.nudged()
    assert its == ref.its and moved < 0.25 * POSE_TOL, (moved, its, ref.its)
    return ref


def _align(p, ncfg, n, init=None, storage=native.STORAGE_F64, batch_invariant=False, slide_off=False, same_frame=False):
    h, w = p["gray0"].shape
    with odometry.AlignmentEngine() as eng:
        if storage != native.STORAGE_F64:
            eng.set_extensions(native.make_extensions(plane_storage=storage))
        eng.set_config(ncfg)
        if batch_invariant:
            eng.set_batch_invariant(True)
        if slide_off:
            eng.set_slide_policy(-1)
        eng.set_intrinsic_matrix(p["K"])
        eng.reserve_frames(2, w, h)
        if same_frame:
            eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_BOTH)
            src, tgt = [0] * n, [0] * n
        else:
            eng.upload_frame(0, p["gray0"], p["depth0"], roles=native.ROLE_SOURCE)
            eng.upload_frame(1, p["gray1"], None, roles=native.ROLE_TARGET)
            src, tgt = [0] * n, [1] * n
        inits = None if init is None else np.tile(np.asarray(init, dtype=np.float64), (n, 1))
        s, reps = eng.align_pairs(src, tgt, init_states=inits, want_reports=True)
        launches = eng.last_launches()
    return s, reps, launches


def _check(ref, states, reps, what):
    """Every pair of a launch against the reference, the figures printed first; every pair of the batch the same bits."""
    nl = len(ref.its)
    for k in range(len(states)):
        d = se3.state_distance(states[k], ref.state)
        gerr = abs(reps[k].gradient_norm - ref.gnorm)
        print(f"pixel loop {what} pair {k}: pose distance {d:.3e}, gradient norm {ref.gnorm:.6e} off by {gerr:.3e}, "
              f"cond {ref.cond:.2e}, valid {ref.valid}, iterations {ref.its}")
        assert list(reps[k].iterations[:nl]) == ref.its, (what, k, list(reps[k].iterations[:nl]), ref.its)
        assert list(reps[k].valid_pixels[:nl]) == ref.valid, (what, k, list(reps[k].valid_pixels[:nl]), ref.valid)
        assert reps[k].flags == 0, (what, k, reps[k].flags)
        assert d <= POSE_TOL, (what, k, d)
        assert gerr <= GRAD_TOL * max(1.0, ref.gnorm), (what, k, reps[k].gradient_norm, ref.gnorm)
        assert np.array_equal(states[k], states[0]) and reps[k].gradient_norm == reps[0].gradient_norm, (what, k)


# ------------------------------------------------------------------------------------------------------------------------
# ownerless rows
# ------------------------------------------------------------------------------------------------------------------------
MOTIONS = {
    "back": (0.0, 0.0, -0.35, 0.0, 0.0, 0.0),           # the ownerless rows lie among the owned ones
    "forth": (0.0, 0.0, 0.35, 0.0, 0.0, 0.0),           # the border rows, first and last chunk included, are all ownerless
}
SPARE_MOTION = (0.02, 0.01, -0.3, 0.03, -0.02, 0.02)    # where the well-posedness rule rejects one of the two at a size
# form -> size, storage, what is set on the engine, (kind, threads) of the first launch
OWNERLESS_FORMS = {
    "one_wave": dict(size=(40, 30), launch=("persistent", 64)),
    "quad_256": dict(size=(80, 60), launch=("persistent", 256)),
    "quad_256_f32": dict(size=(80, 60), storage="f32", launch=("persistent", 256)),
    "quad_256_f16": dict(size=(80, 60), storage="f16", launch=("persistent", 256)),
    "mid_512": dict(size=(128, 96), launch=("persistent", 512)),
    "wide_1024": dict(size=(160, 120), launch=("persistent", 1024)),
    "exact_hbm": dict(size=pb.BEYOND, batch_invariant=True, slide_off=True, launch=("persistent", 1024)),
}
FUSED_SIZE = (160, 120)
MIN_OWNERLESS_SHARE = 0.25


@functools.lru_cache(maxsize=None)
def rendered_pair(size, motion):
    return synthetic.render_pair_with_motion(SEED, size[0], size[1], list(motion))


def init_of(p):
    return p["motion"] + edge_states.NEAR


def ownerless_share(planes, K, state, min_depth=0.3, max_depth=5.0):
    """Of the Jacobian rows one pass fills at `state` on level 0 -- source pixels with a depth inside the gate that land in
    bounds -- the share whose own pixel no source pixel lands on (the scatter of oracle/numpy_twin.normal_equations)."""
    i0, d0 = planes[0][0], planes[1][0]
    H_, W_ = i0.shape
    fx, fy, ox, oy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z, yaw, pitch, roll = state
    sy_, cy_, sp, cp, sr, cr = np.sin(yaw), np.cos(yaw), np.sin(pitch), np.cos(pitch), np.sin(roll), np.cos(roll)
    R = np.array([[cy_ * cp, cy_ * sp * sr - sy_ * cr, cy_ * sp * cr + sy_ * sr],
                  [sy_ * cp, sy_ * sp * sr + cy_ * cr, sy_ * sp * cr - cy_ * sr],
                  [-sp, cp * sr, cp * cr]])
    cc, rr = np.meshgrid(np.arange(W_, dtype=np.float64), np.arange(H_, dtype=np.float64))
    pz = np.asarray(d0, dtype=np.float64).reshape(-1)
    valid = (min_depth < pz) & (pz < max_depth)
    with np.errstate(all="ignore"):
        P = np.stack([(cc.reshape(-1) - ox) * pz / fx, (rr.reshape(-1) - oy) * pz / fy, pz])
        X, Y, Z = R @ P + np.array([[x], [y], [z]])
        tci, tri = numpy_twin.c_round(X * fx / Z + ox), numpy_twin.c_round(Y * fy / Z + oy)
        rows = valid & np.isfinite(tri) & np.isfinite(tci) & (tri >= 0) & (tri < H_) & (tci >= 0) & (tci < W_)
    hit = np.zeros(H_ * W_, dtype=bool)
    hit[(tri[rows] * W_ + tci[rows]).astype(np.int64)] = True
    return float((rows & ~hit).sum()) / float(rows.sum())


@functools.lru_cache(maxsize=None)
def ownerless_case(size, motion_name, storage="f64", levels=1):
    """(pair, reference, share of ownerless rows at the true motion) of one size under one of the two motions -- or under
    the spare motion where the well-posedness rule rejects that one."""
    last = None
    for motion in (MOTIONS[motion_name], SPARE_MOTION):
        p = rendered_pair(size, motion)
        min_grad = None if levels == 1 else [CAP_THRESHOLD] * levels
        _, ocfg = pb.cfgs([ITERS] * levels, min_grad)
        planes = _planes(ocfg, p, STORAGES[storage])
        ref = pb.PhotoRef(ocfg, p["K"], planes, init_of(p))
        try:
            well_posed(ref)
        except AssertionError as e:
            last = e
            continue
        return p, ref, ownerless_share(planes, p["K"], p["motion"])
    raise last


def _ownerless_ids():
    return [(form, name) for form in OWNERLESS_FORMS for name in MOTIONS]


def test_a_quarter_of_the_rows_is_ownerless():
    """(no device work)  Every case's reference is well-posed and at least a quarter of its rows at the true motion has no
    owner; the residuals of the other rows count: no gradient of the trace is small."""
    for form, name in _ownerless_ids():
        f = OWNERLESS_FORMS[form]
        _, ref, share = ownerless_case(f["size"], name, f.get("storage", "f64"))
        print(f"ownerless rows {form} {pb.size_id(f['size'])} {name}: share {share:.3f}, valid {ref.valid}")
        assert share >= MIN_OWNERLESS_SHARE, (form, name, share)
        assert ref.its == [ITERS] and all(g > 1.0 for _, g in ref.gnorms), (form, name, ref.gnorms)
    for name in MOTIONS:
        _, ref, share = ownerless_case(FUSED_SIZE, name, levels=2)
        assert share >= MIN_OWNERLESS_SHARE and ref.its == [ITERS, ITERS], (name, share, ref.its)
        assert all(g > 1000.0 * CAP_THRESHOLD for _, g in ref.gnorms), (name, ref.gnorms)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MOTIONS))
@pytest.mark.parametrize("form", list(OWNERLESS_FORMS))
def test_ownerless_rows_on_every_form(form, name):
    f = OWNERLESS_FORMS[form]
    storage = f.get("storage", "f64")
    p, ref, share = ownerless_case(f["size"], name, storage)
    assert share >= MIN_OWNERLESS_SHARE, share
    ncfg, _ = pb.cfgs([ITERS])
    s, reps, launches = _align(p, ncfg, PAIRS, init_of(p), STORAGES[storage], f.get("batch_invariant", False),
                               f.get("slide_off", False))
    assert [(r["kind"], r["threads"]) for r in launches] == [f["launch"]], (form, launches)
    _check(ref, s, reps, f"ownerless {form} {pb.size_id(f['size'])} {name} share {share:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MOTIONS))
def test_ownerless_rows_in_the_fused_launch(name):
    p, ref, share = ownerless_case(FUSED_SIZE, name, levels=2)
    assert share >= MIN_OWNERLESS_SHARE, share
    ncfg, _ = pb.cfgs([ITERS, ITERS], [CAP_THRESHOLD, CAP_THRESHOLD])
    s, reps, launches = _align(p, ncfg, FUSED_COPIES, init_of(p))
    assert [(r["kind"], r["threads"], r["levels"]) for r in launches] == [("fused", 512, [1, 0])], launches
    _check(ref, s, reps, f"ownerless fused {pb.size_id(FUSED_SIZE)} {name} share {share:.3f}")


# ------------------------------------------------------------------------------------------------------------------------
# every pixel its own owner
# ------------------------------------------------------------------------------------------------------------------------
# the last size of every form with the owner map in LDS (tests/plan_boundaries.py, PHOTO): threads on fp64 planes
OWN_OWNER_SIZES = {(64, 32): 64, (120, 80): 256, (128, 100): 512, (202, 192): 1024}


@functools.lru_cache(maxsize=None)
def own_owner_ref(size, storage):
    """One iteration from the zero state with the source frame as its own target."""
    p = dict(pb.pair(*size))
    p["gray1"] = p["gray0"]
    _, ocfg = pb.cfgs([1])
    ref = pb.PhotoRef(ocfg, p["K"], _planes(ocfg, p, STORAGES[storage]))
    assert ref.finite and ref.its == [1] and ref.gnorm == 0.0 and not np.any(ref.state), (size, ref.gnorm, ref.state)
    return p, ref


def test_the_oracle_finds_nothing_to_move_on_a_frame_against_itself():
    """(no device work)  Every residual of the reference is I(k) - I(k): gradient and step are exactly zero, and nearly
    every pixel with a depth fills a row."""
    for size in OWN_OWNER_SIZES:
        for storage in STORAGES:
            _, ref = own_owner_ref(size, storage)
            assert 10 * ref.valid[0] >= 9 * size[0] * size[1], (size, storage, ref.valid)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("size", list(OWN_OWNER_SIZES), ids=pb.size_id)
def test_every_pixel_its_own_owner(size, storage):
    p, ref = own_owner_ref(size, storage)
    plan = pb.plan_level(size[0] * size[1], bound_by_bytes=storage == "f64")
    assert plan["owner_in_lds"] and (storage != "f64" or plan["threads"] == OWN_OWNER_SIZES[size]), plan
    ncfg, _ = pb.cfgs([1])
    s, reps, launches = _align(p, ncfg, PAIRS, None, STORAGES[storage], same_frame=True)
    assert [(r["kind"], r["threads"]) for r in launches] == [("persistent", plan["threads"])], launches
    for k in range(PAIRS):
        print(f"own owner {pb.size_id(size)} {storage} pair {k}: gradient norm {reps[k].gradient_norm!r}, state {s[k]}, "
              f"valid {reps[k].valid_pixels[0]} (oracle {ref.valid[0]})")
        assert reps[k].gradient_norm == 0.0, (size, storage, reps[k].gradient_norm)
        assert not np.any(s[k]), (size, storage, s[k])
        assert reps[k].iterations[0] == 1 and reps[k].valid_pixels[0] == ref.valid[0] and reps[k].flags == 0, (size, storage)


# ------------------------------------------------------------------------------------------------------------------------
# more than 32 chunks per wave
# ------------------------------------------------------------------------------------------------------------------------
# form -> threads, and three sizes: c = 32 * waves chunks (no wave carries more than 32), c + 1 chunks (wave 0 carries 33),
# c + 1 chunks of which the last is partial
CHUNK_FORMS = {
    "QUAD": dict(threads=256, sizes=((128, 64), (129, 64), (127, 65))),
    "WIDE": dict(threads=1024, sizes=((256, 128), (171, 192), (200, 164))),
    "FUSED": dict(threads=512, sizes=((128, 128), (257, 64), (200, 82))),
}


def _chunk_rows():
    return [(form, size) for form, f in CHUNK_FORMS.items() for size in f["sizes"]]


def _chunk_id(v):
    return pb.size_id(v) if isinstance(v, tuple) else v


@functools.lru_cache(maxsize=None)
def chunk_ref(form, size):
    p = pb.pair(*size)                      # holes of 0.03
    if form == "FUSED":
        _, ocfg = pb.cfgs([ITERS, ITERS], [CAP_THRESHOLD, CAP_THRESHOLD])
        ref = well_posed(pb.PhotoRef(ocfg, p["K"], _pyramids(ocfg, p)))
        assert ref.its == [ITERS, ITERS] and all(g > 1000.0 * CAP_THRESHOLD for _, g in ref.gnorms), (ref.its, ref.gnorms)
        return ref
    return well_posed(pb.photo_ref(size, ITERS))


def test_the_chunk_counts_are_what_they_are_said_to_be():
    """(no device work)  Per form: 32 chunks per wave exactly, then 33 in wave 0, then 33 with a partial last chunk; the
    planner's restatement takes each size in the form named; every reference is well-posed and has holes."""
    for form, f in CHUNK_FORMS.items():
        waves = f["threads"] // pb.WAVE
        ns = [w * h for w, h in f["sizes"]]
        assert [pb.chunks(n) for n in ns] == [32 * waves, 32 * waves + 1, 32 * waves + 1], (form, ns)
        assert ns[0] % pb.WAVE == 0 and ns[1] % pb.WAVE == 0 and ns[2] % pb.WAVE != 0, (form, ns)
        for size, n in zip(f["sizes"], ns):
            if form == "FUSED":
                half = ((size[0] + 1) // 2) * ((size[1] + 1) // 2)
                assert pb.level_fusable(n) and pb.level_fusable(half), (size, n, half)
            else:
                plan = pb.plan_level(n)
                assert (plan["form"], plan["threads"]) == (form, f["threads"]), (size, plan)
            ref = chunk_ref(form, size)
            assert ref.valid[0] < n and 2 * ref.valid[0] >= n, (form, size, ref.valid)


@pytest.mark.gpu
@pytest.mark.parametrize("form,size", _chunk_rows(), ids=_chunk_id)
def test_a_wave_with_more_than_32_chunks(form, size):
    f = CHUNK_FORMS[form]
    p = pb.pair(*size)
    ref = chunk_ref(form, size)
    if form == "FUSED":
        ncfg, _ = pb.cfgs([ITERS, ITERS], [CAP_THRESHOLD, CAP_THRESHOLD])
        s, reps, launches = _align(p, ncfg, FUSED_COPIES)
        assert [(r["kind"], r["threads"], r["levels"]) for r in launches] == [("fused", 512, [1, 0])], launches
    else:
        ncfg, _ = pb.cfgs([ITERS])
        s, reps, launches = _align(p, ncfg, PAIRS)
        assert [(r["kind"], r["threads"]) for r in launches] == [("persistent", f["threads"])], launches
    _check(ref, s, reps, f"chunks {form} {pb.size_id(size)} c {pb.chunks(size[0] * size[1])}")
