"""GPU tests of the device-memory ingest (phovo_engine_upload_frames_device, ingest_kernels.hip).

Every comparison here is EXACT (np.testing.assert_array_equal): the device path packs the caller's frames into the very
staging buffers a host upload fills and then runs the same pyramid producers, so the planes -- and everything computed
from them -- are the host upload's bit for bit.  No tolerance appears in this file.

For float32 / float16 depth the host side uploads depth.astype(float64) * scale computed in numpy: float32 (float16) ->
float64 is exact and one fp64 multiply is correctly rounded on both sides (IEEE 754, no fused form of a lone product), so
these are the same fp64 values the packing kernel stages.

One process, one HIP runtime.  The torch wheel carries its own HIP runtime under an unversioned file name, so a process that
loads libphovo_hip.so (and with it the system's runtime) BEFORE it imports torch ends up with two runtimes, the second of
which sees no device; imported first, torch's runtime is the one the library binds to as well, and tensors and engine share
it.  A torch user imports torch first by nature.  A pytest session that ran other GPU tests of this suite before this
file has the library loaded already, so every test below runs in ONE child pytest process of this file that imports torch
before anything else (PHOVO_INGEST_TEST_CHILD=1); the test of the same name in the parent session reports that child
test's outcome -- passed, failed with the child's message, or skipped -- and computes nothing itself."""
import ctypes as C
import functools
import inspect
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

CHILD = os.environ.get("PHOVO_INGEST_TEST_CHILD") == "1"
if CHILD:
    import torch as _torch_first  # noqa: F401  (before libphovo_hip.so is loaded: see the module docstring)

import numpy as np  # noqa: E402
import pytest  # noqa: E402

import phovo_amd  # noqa: E402,F401
from phovo_amd import native, odometry, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "apps", "bin", "png_probe")
TUM = 1.0 / 5000.0
BLURS = {"off": [0, 0, 0, 0], "level0": [3, 0, 0, 0], "every": [3, 5, 3, 3]}
ROLES = {"source": native.ROLE_SOURCE, "target": native.ROLE_TARGET, "both": native.ROLE_BOTH}


@pytest.fixture(scope="module")
def child_results(tmp_path_factory):
    """Parent session: runs this file once in a child pytest process and returns {test id: (outcome, text)}."""
    if CHILD:
        return None
    xml = tmp_path_factory.mktemp("device_ingest") / "child.xml"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                        f"--junitxml={xml}"], cwd=ROOT, env=dict(os.environ, PHOVO_INGEST_TEST_CHILD="1"),
                       capture_output=True, text=True, timeout=1200)
    assert os.path.exists(xml), "the child pytest process wrote no report:\n" + (r.stdout + r.stderr)[-4000:]
    out = {}
    for case in ET.parse(xml).getroot().iter("testcase"):
        bad = [c for c in case if c.tag in ("failure", "error")]
        skipped = [c for c in case if c.tag == "skipped"]
        text = "\n".join((c.get("message") or "") + "\n" + (c.text or "") for c in bad + skipped)
        out[case.get("name")] = ("failed" if bad else "skipped" if skipped else "passed", text)
    return out


def in_child(fn):
    """The test body runs in the child process; in the parent session the test reports the child's outcome."""
    sig = inspect.signature(fn)
    extra = [inspect.Parameter(n, inspect.Parameter.POSITIONAL_OR_KEYWORD) for n in ("request", "child_results")
             if n not in sig.parameters]

    @functools.wraps(fn)
    def wrapper(*args, request, child_results, **kwargs):
        if CHILD:
            return fn(*args, **kwargs)
        outcome, text = child_results.get(request.node.name, ("failed", "the child process did not run this test"))
        if outcome == "skipped":
            pytest.skip(text.strip().splitlines()[0] if text.strip() else "skipped in the child process")
        assert outcome == "passed", text

    wrapper.__signature__ = sig.replace(parameters=list(sig.parameters.values()) + extra)
    return wrapper


@pytest.fixture(scope="module")
def torch():
    if not CHILD:
        return None
    import torch
    return torch


def _engine(storage=native.STORAGE_F64, blur="off", objective=native.OBJECTIVE_PHOTOMETRIC,
            sampling=native.SAMPLING_NEAREST_SCATTER, max_iter=(2, 2, 2, 2), K=None, levels=4):
    e = odometry.AlignmentEngine(0)
    e.set_extensions(native.make_extensions(plane_storage=storage, sampling=sampling))
    e.set_config(native.make_config(num_levels=levels, blur=BLURS[blur][:levels], max_iter=list(max_iter)[:levels],
                                    min_grad=[1.0] * levels))
    if objective != native.OBJECTIVE_PHOTOMETRIC:
        e.set_objective(objective)
    e.set_intrinsic_matrix(K if K is not None else np.array([[525., 0, 319.5], [0, 525., 239.5], [0, 0, 1]]))
    return e


def _frames(seed, n, w, h):
    """gray u8 [n,h,w] and raw depth samples u16 [n,h,w] with holes (0 = invalid)."""
    rng = np.random.default_rng(seed)
    gray = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    raw = rng.integers(1500, 25000, (n, h, w)).astype(np.uint16)
    raw[rng.random((n, h, w)) < 0.1] = 0
    return gray, raw


def _depth_forms(kind, raw, torch):
    """(host upload kwargs, device tensor, device depth_scale) of one depth format, from raw u16 samples."""
    if kind == "f64":
        d = raw.astype(np.float64) * TUM + 1e-3 * np.sin(raw.astype(np.float64))       # any fp64 values
        return dict(depth=d), torch.from_numpy(d).cuda(), 1.0
    if kind == "u16":
        return dict(depth=raw, depth_scale=TUM), torch.from_numpy(raw.view(np.int16)).cuda().view(torch.uint16), TUM
    if kind == "f32":
        v = (raw.astype(np.float32) * np.float32(1.0009765625)).astype(np.float32)
        return dict(depth=v.astype(np.float64) * TUM), torch.from_numpy(v).cuda(), TUM
    assert kind == "f16"
    v = (raw.astype(np.float32) / np.float32(4096.0)).astype(np.float16)                # metres-ish, in fp16 range
    scale = 0.9987
    return dict(depth=v.astype(np.float64) * scale), torch.from_numpy(v).cuda(), scale


def _all_planes(e, frames, bi=False):
    out = []
    for f in frames:
        for level in range(e.get_config().num_levels):
            if not e.level_is_stored(level):
                continue
            out.extend(e.get_level_planes(f, level))
            if bi:
                out.extend(e.get_level_depth_gradients(f, level))
                out.append(np.array([e.get_level_depth_gain(f, level)]))
    assert out
    return out


def _assert_same_planes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _host_vs_device(torch, eh, ed, roles, kind, w, h, first, count, seed=0):
    """The same frames through upload_frames into eh and through upload_frames_device into ed (two engines with the same
    settings, pools reserved anew): every stored level, all four planes, of every pool slot."""
    gray, raw = _frames(seed, count, w, h)
    host_kw, d_dev, scale = _depth_forms(kind, raw, torch)
    n = first + count + 1
    eh.reserve_frames(n, w, h)
    ed.reserve_frames(n, w, h)
    eh.upload_frames(first, gray, roles=roles, **host_kw)
    ed.upload_frames_device(first, torch.from_numpy(gray).cuda(), d_dev, depth_scale=scale, roles=roles)
    rec = ed.last_ingest()
    assert rec["chunks"] == (count + 31) // 32
    want_wide = w % 16 == 0
    assert (rec["wide_launches"] > 0) == want_wide and (rec["scalar_launches"] > 0) == (not want_wide), rec
    for f in range(n):                                    # (frame by frame: 73 frames of 640x480 are a gigabyte of planes)
        _assert_same_planes(_all_planes(eh, [f]), _all_planes(ed, [f]))


# ---- 1. planes equal the host upload's ------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", [native.STORAGE_F64, native.STORAGE_F32, native.STORAGE_F16])
@pytest.mark.parametrize("blur", list(BLURS))
@pytest.mark.parametrize("kind", ["f64", "u16", "f32", "f16"])
@in_child
def test_planes_equal_the_host_uploads_every_storage_blur_and_depth_format(torch, storage, blur, kind):
    """Every stored level, all four planes, every role, on 161x119 (scalar form: odd width) with first_frame > 0."""
    with _engine(storage, blur) as eh, _engine(storage, blur) as ed:
        for i, roles in enumerate(ROLES.values()):
            _host_vs_device(torch, eh, ed, roles, kind, 161, 119, first=1 + i, count=2, seed=10 * i + storage)


@pytest.mark.parametrize("w,h", [(640, 480), (161, 119), (5, 3)])
@pytest.mark.parametrize("count", [1, 33, 70])
@in_child
def test_planes_equal_the_host_uploads_every_size_and_chunking(torch, w, h, count):
    """count 33 crosses a chunk boundary, 70 uses both staging halves twice; 640x480 takes the wide form."""
    kind = {1: "f32", 33: "u16", 70: "f64"}[count] if w != 161 else {1: "f16", 33: "f32", 70: "u16"}[count]
    storage = {640: native.STORAGE_F64, 161: native.STORAGE_F16, 5: native.STORAGE_F32}[w]
    blur = "off" if count == 70 else "every"
    levels = 2 if w == 5 else 4                           # (5x3 has no third level: 1x1, then a height of 0)
    with _engine(storage, blur, levels=levels) as eh, _engine(storage, blur, levels=levels) as ed:
        _host_vs_device(torch, eh, ed, native.ROLE_BOTH, kind, w, h, first=2, count=count, seed=count)


@pytest.mark.parametrize("roles", list(ROLES))
@pytest.mark.parametrize("kind", ["f64", "u16", "f32", "f16"])
@in_child
def test_planes_equal_the_host_uploads_full_size_every_role_and_format(torch, roles, kind):
    with _engine(native.STORAGE_F64, "level0") as eh, _engine(native.STORAGE_F64, "level0") as ed:
        _host_vs_device(torch, eh, ed, ROLES[roles], kind, 640, 480, first=1, count=3, seed=5)


# ---- 2. strides -------------------------------------------------------------------------------------------------------

@in_child
def test_strided_views_give_the_planes_of_the_contiguous_copy_in_both_kernel_forms(torch):
    """Row padding, frame padding, a 3-channel view and an offset start that breaks 16-byte alignment.  The launch record
    (last_ingest) shows that the aligned views took the wide form and the misaligned ones the scalar form."""
    w, h, n = 64, 24, 3
    rng = np.random.default_rng(3)
    big_g = torch.from_numpy(rng.integers(0, 256, (2 * n, h + 3, w + 48), dtype=np.uint8)).cuda()
    big_c = torch.from_numpy(rng.integers(0, 256, (2 * n, h + 3, w + 48, 3), dtype=np.uint8)).cuda()
    big_d = {"f64": torch.from_numpy(rng.random((2 * n, h + 3, w + 48)) * 4).cuda(),
             "f32": torch.from_numpy((rng.random((2 * n, h + 3, w + 48)) * 4).astype(np.float32)).cuda(),
             "f16": torch.from_numpy((rng.random((2 * n, h + 3, w + 48)) * 4).astype(np.float16)).cuda(),
             "u16": torch.from_numpy(rng.integers(0, 30000, (2 * n, h + 3, w + 48)).astype(np.int16)).cuda().view(torch.uint16)}
    seen = {"wide": 0, "scalar": 0}
    cases = [(x0, want, colour, kind) for x0, want in ((16, "wide"), (0, "wide"), (3, "scalar"), (1, "scalar"))
             for colour in (False, True) for kind in big_d]
    with _engine() as ev, _engine() as ec:
        for x0, want, colour, kind in cases:
            bd = big_d[kind]
            src = big_c if colour else big_g
            gv = src[::2, 1:1 + h, x0:x0 + w]                      # frame padding, row padding, offset start
            dv = bd[::2, 2:2 + h, x0:x0 + w]
            assert not gv.is_contiguous() and not dv.is_contiguous()
            gi, di, keep, shape, _ = odometry._device_images(gv, dv, "rgb", None, 0, batched=True)
            assert gi.data == gv.data_ptr() and di.data == dv.data_ptr(), "a strided view must be passed through, not copied"
            assert shape == (n, h, w)
            scale = 1.0 if kind == "f64" else 0.5
            ev.reserve_frames(n, w, h)
            ec.reserve_frames(n, w, h)
            ev.upload_frames_device(0, gv, dv, depth_scale=scale)
            rec_v = ev.last_ingest()
            ec.upload_frames_device(0, gv.contiguous(), dv.contiguous(), depth_scale=scale)
            rec_c = ec.last_ingest()
            _assert_same_planes(_all_planes(ev, range(n)), _all_planes(ec, range(n)))
            # u16 / f16 at an odd pixel offset are still only 2-byte aligned, u8 at offset 3 or 1 is 1-byte aligned...
            if want == "wide":
                assert rec_v == dict(chunks=1, wide_launches=2, scalar_launches=0), (x0, colour, kind, rec_v)
            else:
                assert rec_v["scalar_launches"] >= 1, (x0, colour, kind, rec_v)
            assert rec_c == dict(chunks=1, wide_launches=2, scalar_launches=0), rec_c
            seen["wide"] += rec_v["wide_launches"]
            seen["scalar"] += rec_v["scalar_launches"]
    assert seen["wide"] > 0 and seen["scalar"] > 0


@in_child
def test_a_pixel_stride_is_the_only_thing_that_costs_a_copy(torch):
    w, h = 32, 8
    g = torch.zeros((2, h, 2 * w), dtype=torch.uint8, device="cuda")[:, :, ::2]          # pixel stride 2
    gi, _, keep, _, _ = odometry._device_images(g, None, "rgb", None, 0, batched=True)
    assert gi.data != g.data_ptr() and keep[0].is_contiguous()
    c = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda")[..., :3]              # RGBA storage: pixel stride 4
    gi, _, keep, _, _ = odometry._device_images(c, None, "rgb", None, 0, batched=True)
    assert gi.data != c.data_ptr() and gi.row_stride_bytes == 3 * w


# ---- 3. colour --------------------------------------------------------------------------------------------------------

def _level0_bytes(e, frame):
    plane = e.get_level_planes(frame, 0)[0]
    b = np.rint(plane * 255.0)
    np.testing.assert_array_equal(b * (1.0 / 255), plane)                 # the plane is exactly byte * (1./255)
    return b.astype(np.uint8)


@pytest.fixture(scope="module")
def png_probe():
    if not CHILD:
        return None
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps"), PROBE])
    return PROBE


@in_child
def test_rgb_and_bgr_reduce_to_gray_by_the_projects_integer_rule(torch, png_probe, tmp_path):
    from PIL import Image
    w, h = 48, 20
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8)
    rgb[2].reshape(-1, 3)[:8] = corners
    want = ((9797 * rgb[..., 0].astype(np.int64) + 19234 * rgb[..., 1].astype(np.int64) + 3737 * rgb[..., 2].astype(np.int64)
             + 16384) >> 15).astype(np.uint8)
    np.testing.assert_array_equal(want, odometry.gray_from_colour(rgb, "rgb"))
    np.testing.assert_array_equal(want, odometry.gray_from_colour(rgb[..., ::-1], "bgr"))
    assert want[2].reshape(-1)[0] == 0 and want[2].reshape(-1)[7] == 255
    with _engine() as e, _engine() as eh:
        e.reserve_frames(6, w, h)
        eh.reserve_frames(6, w, h)
        e.upload_frames_device(0, torch.from_numpy(rgb).cuda(), roles=native.ROLE_TARGET, channel_order="rgb")
        e.upload_frames_device(3, torch.from_numpy(rgb[..., ::-1].copy()).cuda(), roles=native.ROLE_TARGET, channel_order="bgr")
        eh.upload_frames(0, want, roles=native.ROLE_TARGET)
        eh.upload_frames(3, want, roles=native.ROLE_TARGET)
        _assert_same_planes(_all_planes(e, range(6)), _all_planes(eh, range(6)))
        for f in range(3):
            np.testing.assert_array_equal(_level0_bytes(e, f), want[f])
            np.testing.assert_array_equal(_level0_bytes(e, 3 + f), want[f])
    # the same pixels through the PNG reader of the apps (read_gray8)
    Image.fromarray(rgb[2], "RGB").save(tmp_path / "c.png")
    subprocess.check_call([png_probe, "gray8", str(tmp_path / "c.png"), str(tmp_path / "c.raw")])
    with open(tmp_path / "c.raw", "rb") as f:
        pw, ph = [int(v) for v in f.readline().split()]
        from_png = np.frombuffer(f.read(), dtype=np.uint8).reshape(ph, pw)
    np.testing.assert_array_equal(from_png, want[2])


# ---- 4. every objective sees the same frames --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pairs():
    if not CHILD:
        return None
    return [synthetic.make_pair(s, 320, 240, holes=0.05 if s % 2 else 0.0) for s in range(3)]


def _upload_pairs(e, ps, torch, device):
    g = np.stack([p[k] for p in ps for k in ("gray0", "gray1")])
    d = np.stack([p[k] for p in ps for k in ("depth0", "depth1")])
    e.reserve_frames(len(g), g.shape[2], g.shape[1])
    if device:
        e.upload_frames_device(0, torch.from_numpy(g).cuda(), torch.from_numpy(d).cuda())
    else:
        e.upload_frames(0, g, d)


@pytest.mark.parametrize("name", ["photometric", "bilinear_fp16", "biobjective", "trust_region"])
@in_child
def test_every_objective_aligns_device_ingested_frames_to_the_same_bits(torch, pairs, name):
    kw = {"photometric": dict(),
          "bilinear_fp16": dict(storage=native.STORAGE_F16, sampling=native.SAMPLING_BILINEAR),
          "biobjective": dict(objective=native.OBJECTIVE_BIOBJECTIVE),
          "trust_region": dict(objective=native.OBJECTIVE_TRUST_REGION)}[name]
    K = pairs[0]["K"]
    src, tgt = [0, 2, 4], [1, 3, 5]
    with _engine(max_iter=(0, 3, 5, 8), K=K, **kw) as eh, _engine(max_iter=(0, 3, 5, 8), K=K, **kw) as ed:
        _upload_pairs(eh, pairs, torch, device=False)
        _upload_pairs(ed, pairs, torch, device=True)
        bi = name == "biobjective"
        # aligned first: no host synchronisation has happened between the ingest and this enqueue
        sd, rd = ed.align_pairs(src, tgt, want_reports=True)
        sh, rh = eh.align_pairs(src, tgt, want_reports=True)
        np.testing.assert_array_equal(sd, sh)
        assert np.all(np.isfinite(sh)) and np.any(sh != 0)
        for a, b in zip(rd, rh):
            assert list(a.iterations) == list(b.iterations) and list(a.valid_pixels) == list(b.valid_pixels)
            assert a.gradient_norm == b.gradient_norm and a.flags == b.flags
        _assert_same_planes(_all_planes(eh, range(6), bi), _all_planes(ed, range(6), bi))
        if name == "photometric":
            for level in (1, 3):
                a = ed.evaluate_pairs(src, tgt, sd, level)
                b = eh.evaluate_pairs(src, tgt, sh, level)
                for key in ("information", "gradient", "cost", "rows", "flags"):
                    np.testing.assert_array_equal(a[key], b[key])


@in_child
def test_evaluate_pairs_right_after_an_ingest_is_ordered_behind_it(torch, pairs):
    K = pairs[0]["K"]
    states = np.zeros((3, 6))
    with _engine(K=K) as eh, _engine(K=K) as ed:
        _upload_pairs(eh, pairs, torch, device=False)
        _upload_pairs(ed, pairs, torch, device=True)
        a = ed.evaluate_pairs([0, 2, 4], [1, 3, 5], states, 0)
        b = eh.evaluate_pairs([0, 2, 4], [1, 3, 5], states, 0)
        for key in ("information", "gradient", "cost", "rows", "flags"):
            np.testing.assert_array_equal(a[key], b[key])


# ---- 5. ordering ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [8, 64])
@in_child
def test_the_ingest_is_ordered_behind_the_producer_and_the_producer_behind_the_read(torch, count):
    """(a) the tensors are filled by torch kernels on a side stream and handed over with that stream, unsynchronised;
    (b) the same tensors are overwritten on that stream right after the call returns.  The planes are those of the first
    contents.  64 frames: two chunks."""
    w, h = 640, 480
    g1, r1 = _frames(21, count, w, h)
    g2, r2 = _frames(22, count, w, h)
    a_g, a_d = torch.from_numpy(g1).cuda(), torch.from_numpy(r1.view(np.int16)).cuda()
    b_g, b_d = torch.from_numpy(g2).cuda(), torch.from_numpy(r2.view(np.int16)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with _engine() as eh, _engine() as ed:
        eh.reserve_frames(count, w, h)
        ed.reserve_frames(count, w, h)
        eh.upload_frames(0, g1, r1, depth_scale=TUM)
        # staging is allocated by the first ingest (a host wait): do one before the race so that the timed one has none
        ed.upload_frames_device(0, b_g, b_d.view(torch.uint16), depth_scale=TUM)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            tg = torch.empty_like(a_g)
            td = torch.empty_like(a_d)
            tg.copy_(a_g, non_blocking=True)
            td.copy_(a_d, non_blocking=True)
            ed.upload_frames_device(0, tg, td.view(torch.uint16), depth_scale=TUM, stream=side)
            tg.copy_(b_g, non_blocking=True)
            td.copy_(b_d, non_blocking=True)
        _assert_same_planes(_all_planes(eh, range(count)), _all_planes(ed, range(count)))
        side.synchronize()
        np.testing.assert_array_equal(tg.cpu().numpy(), g2)          # and the overwrite did happen, afterwards


# ---- 6. refusals ------------------------------------------------------------------------------------------------------

def _image(t, fmt, row=None, frame=None, reserved=0, data=None):
    es = t.element_size()
    return native.DeviceImage(t.data_ptr() if data is None else data, t.stride(1) * es if row is None else row,
                              t.stride(0) * es if frame is None else frame, fmt, reserved)


def _refused(e, status, needle, first, count, roles, gi, di, scale=1.0):
    L = native.lib()
    st = L.phovo_engine_upload_frames_device(e._h if e is not None else None, first, count, roles,
                                             C.byref(gi) if gi is not None else None,
                                             C.byref(di) if di is not None else None, scale, None)
    msg = L.phovo_last_error().decode()
    assert st == status, (st, msg)
    assert needle in msg, (needle, msg)


@in_child
def test_refusals_name_the_argument_and_leave_the_pool_untouched(torch):
    w, h, n = 32, 12, 4
    gray, raw = _frames(31, n, w, h)
    g = torch.from_numpy(gray).cuda()
    d = torch.from_numpy(raw.astype(np.float32)).cuda()
    d64 = d.double()
    c = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    IA = native.E_INVALID_ARGUMENT
    with _engine() as e:
        _refused(e, native.E_NOT_READY, "reserve_frames", 0, 1, 3, _image(g, native.IMAGE_U8_GRAY), _image(d, native.IMAGE_F32))
        e.reserve_frames(n, w, h)
        e.upload_frames(0, gray, raw, depth_scale=TUM)
        before = _all_planes(e, range(n))
        gi, di = _image(g, native.IMAGE_U8_GRAY), _image(d, native.IMAGE_F32)
        _refused(None, IA, "null engine", 0, 1, 3, gi, di)
        _refused(e, IA, "intensity", 0, 1, 3, None, di)
        _refused(e, IA, "depth is null", 0, 1, native.ROLE_SOURCE, gi, None)
        _refused(e, IA, "first_frame", n - 1, 2, 3, gi, di)
        _refused(e, IA, "first_frame", -1, 1, 3, gi, di)
        _refused(e, IA, "roles", 0, 1, 0, gi, di)
        _refused(e, IA, "intensity.format", 0, 1, 3, _image(g, 99), di)
        _refused(e, IA, "intensity.format", 0, 1, 3, _image(g, native.IMAGE_U16), di)
        _refused(e, IA, "depth.format", 0, 1, 3, gi, _image(d, native.IMAGE_U8_GRAY))
        _refused(e, IA, "depth.format", 0, 1, 3, gi, _image(d, -1))
        _refused(e, IA, "intensity.row_stride_bytes", 0, 1, 3, _image(g, native.IMAGE_U8_GRAY, row=w - 1), di)
        _refused(e, IA, "intensity.row_stride_bytes", 0, 1, 3, _image(c, native.IMAGE_U8_RGB, row=w), di)
        _refused(e, IA, "depth.row_stride_bytes", 0, 1, 3, gi, _image(d, native.IMAGE_F32, row=4 * w - 4))
        _refused(e, IA, "intensity.frame_stride_bytes", 0, 2, 3, _image(g, native.IMAGE_U8_GRAY, frame=w * h - 1), di)
        _refused(e, IA, "depth.frame_stride_bytes", 0, 2, 3, gi, _image(d, native.IMAGE_F32, frame=0))
        _refused(e, IA, "intensity.reserved", 0, 1, 3, _image(g, native.IMAGE_U8_GRAY, reserved=1), di)
        _refused(e, IA, "depth.reserved", 0, 1, 3, gi, _image(d, native.IMAGE_F32, reserved=-7))
        _refused(e, IA, "depth_scale", 0, 1, 3, gi, di, scale=float("nan"))
        _refused(e, IA, "depth_scale", 0, 1, 3, gi, di, scale=float("inf"))
        _refused(e, IA, "depth_scale", 0, 1, 3, gi, _image(d64, native.IMAGE_F64), scale=2.0)
        # host memory: page-locked (the runtime knows it, as host memory) and a plain numpy buffer (it does not)
        pinned = torch.from_numpy(gray).pin_memory()
        _refused(e, IA, "intensity.data", 0, 1, 3, _image(pinned, native.IMAGE_U8_GRAY), di)
        _refused(e, IA, "intensity.data", 0, 1, 3, _image(g, native.IMAGE_U8_GRAY, data=gray.ctypes.data), di)
        dp = torch.from_numpy(raw.astype(np.float32)).pin_memory()
        _refused(e, IA, "depth.data", 0, 1, 3, gi, _image(dp, native.IMAGE_F32))
        _refused(e, IA, "intensity.data", 0, 1, 3, _image(g, native.IMAGE_U8_GRAY, data=0), di)
        # more frames than the allocation holds
        _refused(e, IA, "intensity.data", 0, n, 3, _image(g, native.IMAGE_U8_GRAY, frame=1 << 30), di)
        _assert_same_planes(before, _all_planes(e, range(n)))
        # and the wrapper's own refusals
        with pytest.raises(TypeError):
            e.upload_frames_device(0, torch.from_numpy(gray), d)
        with pytest.raises(TypeError):
            e.upload_frames_device(0, gray, d)
        with pytest.raises(TypeError):
            e.upload_frames_device(0, g, d.to(torch.bfloat16))
        with pytest.raises(ValueError):
            e.upload_frames_device(0, g[:, :, :16], d[:, :, :16])
        _assert_same_planes(before, _all_planes(e, range(n)))
    with _engine(objective=native.OBJECTIVE_BIOBJECTIVE) as e:
        e.reserve_frames(n, w, h)
        before = _all_planes(e, range(n), bi=True)
        _refused(e, IA, "depth is null", 0, 1, native.ROLE_TARGET, _image(g, native.IMAGE_U8_GRAY), None)
        _assert_same_planes(before, _all_planes(e, range(n), bi=True))


@in_child
def test_a_tensor_of_another_device_is_refused(torch):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    w, h = 32, 12
    gray, raw = _frames(32, 1, w, h)
    g = torch.from_numpy(gray).to("cuda:1")
    d = torch.from_numpy(raw.astype(np.float32)).to("cuda:1")
    with _engine() as e:
        e.reserve_frames(1, w, h)
        before = _all_planes(e, [0])
        _refused(e, native.E_INVALID_ARGUMENT, "belongs to device 1", 0, 1, 3, _image(g, native.IMAGE_U8_GRAY),
                 _image(d, native.IMAGE_F32))
        _assert_same_planes(before, _all_planes(e, [0]))


# ---- 7. class surface -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", ["Analytic", "BiObjective", "Ceres"])
@in_child
def test_set_frame_device_on_the_classes_equals_set_frame(torch, pairs, cls):
    p = pairs[1]
    klass = getattr(odometry, "CPhotoconsistencyOdometry" + cls)
    cfg = native.make_config(num_levels=4, max_iter=[0, 3, 5, 8], min_grad=[1.0] * 4)
    results = []
    for device in (False, True):
        with klass(0) as po:
            po.SetConfiguration(cfg)
            po.SetIntrinsicMatrix(p["K"])
            if device:
                po.SetSourceFrameDevice(torch.from_numpy(p["gray0"]).cuda(), torch.from_numpy(p["depth0"]).cuda())
                po.SetTargetFrameDevice(torch.from_numpy(p["gray1"]).cuda(), torch.from_numpy(p["depth1"]).cuda())
            else:
                po.SetSourceFrame(p["gray0"], p["depth0"])
                po.SetTargetFrame(p["gray1"], p["depth1"])
            po.SetInitialStateVector(np.zeros(6))
            po.Optimize()
            rep = po.GetReport()
            results.append((po.GetOptimalStateVector(), list(rep.iterations), list(rep.valid_pixels), rep.gradient_norm))
            if device and cls == "Analytic":
                po.GetPairSystem()                                         # available after Optimize() ...
                po.SetTargetFrameDevice(torch.from_numpy(p["gray1"]).cuda())
                with pytest.raises(native.PhovoError) as ei:               # ... and dropped by Set*FrameDevice, as by Set*Frame
                    po.GetPairSystem()
                assert ei.value.status == native.E_NOT_READY
                po.Optimize()
                po.GetPairSystem()
                po.SetSourceFrameDevice(torch.from_numpy(p["gray0"]).cuda(), torch.from_numpy(p["depth0"]).cuda())
                with pytest.raises(native.PhovoError) as ei:
                    po.GetPairSystem()
                assert ei.value.status == native.E_NOT_READY
    np.testing.assert_array_equal(results[0][0], results[1][0])
    assert results[0][1:] == results[1][1:]
    assert np.any(results[0][0] != 0)


@in_child
def test_set_frame_device_takes_f32_depth_and_colour(torch, pairs):
    p = pairs[0]
    rgb = np.repeat(p["gray0"][..., None], 3, axis=2)
    rgb[..., 0] ^= 0x15
    d32 = p["depth0"].astype(np.float32)
    cfg = native.make_config(num_levels=4, max_iter=[0, 3, 5, 8], min_grad=[1.0] * 4)
    states = []
    for device in (False, True):
        with odometry.CPhotoconsistencyOdometryAnalytic(0) as po:
            po.SetConfiguration(cfg)
            po.SetIntrinsicMatrix(p["K"])
            if device:
                po.SetSourceFrameDevice(torch.from_numpy(rgb[..., ::-1].copy()).cuda(), torch.from_numpy(d32).cuda(),
                                        depth_scale=1.5, channel_order="bgr")
                po.SetTargetFrameDevice(torch.from_numpy(p["gray1"]).cuda())
            else:
                po.SetSourceFrame(odometry.gray_from_colour(rgb), d32.astype(np.float64) * 1.5)
                po.SetTargetFrame(p["gray1"])
            po.Optimize()
            states.append(po.GetOptimalStateVector())
    np.testing.assert_array_equal(states[0], states[1])
