"""k_warp_scatter / k_warp_gather / phovo_warp_image (csrc/warp_kernels.hip) at their edges; run with -m gpu on an MI355X.

* every exact problem of tests/warp_cases.py through phovo_warp_image and through odometry.warpImage: equal to its closed
  form (which tests/test_warp_cases_cpu.py holds to the oracle and the reference build without a device), then to the
  oracle; run twice with identical bits and untouched inputs;
* the grid-stride shape, 1025 x 1024 = 1,049,600 pixels: both kernels cap their grid at 4096 workgroups of 256 threads, so
  the last 1024 pixels are the first ever to take the loop's second trip;
* the 64 draws of the sweep against the oracle, exact;
* strides longer than the rows, refusals (a good call after each), and odometry.warpImage's conversions.
Every directed case asserts that it reached its edge (Problem.reached, computed in exact rational arithmetic).
"""
import ctypes as C

import numpy as np
import pytest

import warp_cases as wc

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry
from oracle import oracle

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
E_INVALID_ARGUMENT, E_SHAPE, E_HIP = 1, 3, 4


def _raw(gray, depth, rt, K, level, w, h, out, device=0, strides=None, null=None):
    """phovo_warp_image itself; `strides` overrides (gray, depth, out) byte strides, `null` names one pointer to pass as NULL."""
    rtf, kf = np.ascontiguousarray(rt, dtype=np.float64).reshape(16), np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    gs, ds, os_ = strides or (gray.strides[0], depth.strides[0], out.strides[0])
    ptr = {"gray": gray.ctypes.data, "depth": depth.ctypes.data, "rt": rtf.ctypes.data_as(DP), "k": kf.ctypes.data_as(DP),
           "out": out.ctypes.data}
    if null:
        ptr[null] = None
    return native.lib().phovo_warp_image(device, ptr["gray"], gs, ptr["depth"], ds, w, h, ptr["rt"], ptr["k"], level,
                                         ptr["out"], os_)


def _run_problem(p):
    assert all(p.reached.values()), (p.name, [k for k, v in p.reached.items() if not v])
    gray, depth, rt, K = p.gray.copy(), p.depth.copy(), p.rt.copy(), p.K.copy()
    outs = []
    for fill in (0x5A, 0xA5):                                       # twice, over different garbage
        out = np.full((p.h, p.w), fill, dtype=np.uint8)
        assert _raw(gray, depth, rt, K, p.level, p.w, p.h, out) == 0, native.lib().phovo_last_error()
        outs.append(out)
    via = odometry.warpImage(gray, depth, rt, K, level=p.level)
    assert np.array_equal(outs[0], p.expected), (p.name, np.argwhere(outs[0] != p.expected)[:8])
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(via, outs[0]), p.name
    assert np.array_equal(outs[0], oracle.warp_image(p.gray, p.depth, p.rt, p.K, p.level)), p.name
    assert np.array_equal(gray, p.gray) and np.array_equal(depth, p.depth, equal_nan=True), p.name
    assert np.array_equal(rt, p.rt) and np.array_equal(K, p.K), p.name


KINDS = ["behind", "collapse", "gate", "halving", "identity", "inf_depth", "invalid", "shift", "subnormal_depth", "z_tiny",
         "z_zero"]


def test_every_kind_is_listed():
    assert KINDS == sorted({p.kind for p in wc.small_problems()})


@pytest.mark.parametrize("kind", KINDS)
def test_exact_problems(kind):
    ps = [p for p in wc.small_problems() if p.kind == kind]
    assert ps
    for p in ps:
        _run_problem(p)


@pytest.mark.parametrize("index", range(4), ids=["identity", "collapse", "half_column", "half_column_and_row"])
def test_grid_stride_second_trip(index):
    """1,049,600 pixels: pixels 1,048,576 and up are reached only by the second trip of `i += gridDim.x * blockDim.x`."""
    assert len(wc.big_problems()) == 4
    p = wc.big_problems()[index]
    assert p.w * p.h > wc.GRID_STRIDE and int(p.owner.max()) >= wc.GRID_STRIDE
    _run_problem(p)
    if p.kind == "identity":
        assert np.array_equal(p.expected[-1], p.gray[-1])           # the last row, the second trip's, included


@pytest.mark.parametrize("first", range(0, wc.SWEEP_DRAWS, 8))
def test_sweep(first):
    for i in range(first, first + 8):
        d = wc.sweep_draw(i)
        exp = oracle.warp_image(d["gray"], d["depth"], d["rt"], d["K"], d["level"])
        got = odometry.warpImage(d["gray"], d["depth"], d["rt"], d["K"], level=d["level"])
        assert np.array_equal(got, exp), (i, d["stats"], np.argwhere(got != exp)[:8])
        again = odometry.warpImage(d["gray"], d["depth"], d["rt"], d["K"], level=d["level"])
        assert np.array_equal(got, again), i


def _padded(p, pads):
    """The problem's planes inside wider ones; the padding holds values that would show if it were read as image."""
    pg, pd, po = pads
    g = np.full((p.h, p.w + pg), 255, dtype=np.uint8)
    d = np.full((p.h, p.w + pd), 1.5)
    g[:, :p.w], d[:, :p.w] = p.gray, p.depth
    return g, d, np.full((p.h, p.w + po), 77, dtype=np.uint8)


@pytest.mark.parametrize("pads", [(11, 0, 0), (0, 5, 0), (0, 0, 3), (1, 2, 7)], ids=["gray", "depth", "out", "all"])
@pytest.mark.parametrize("big", [False, True], ids=["255px", "grid_stride"])
def test_strides_longer_than_the_rows(big, pads):
    p = wc.big_problems()[3] if big else next(q for q in wc.small_problems() if q.name == "shift_+0.5_+0.5_15x17_L0")
    assert (p.w * p.h > wc.GRID_STRIDE) if big else (p.w * p.h < 256)
    assert p.kind == "shift" and p.expected.any()
    g, d, out = _padded(p, pads)
    assert _raw(g, d, p.rt, p.K, p.level, p.w, p.h, out) == 0, native.lib().phovo_last_error()
    assert np.array_equal(out[:, :p.w], p.expected)
    assert np.all(out[:, p.w:] == 77)                                # the output's padding keeps its fill


def _good_call_still_works():
    p = next(q for q in wc.small_problems() if q.name == "halving_32x16_L0")
    out = np.full((p.h, p.w), 9, dtype=np.uint8)
    assert _raw(p.gray, p.depth, p.rt, p.K, 0, p.w, p.h, out) == 0
    assert np.array_equal(out, p.expected)


def test_refusals():
    L = native.lib()
    w, h = 8, 4
    g, d, out = wc.gray_ramp(w, h), np.ones((h, w)), np.full((h, w), 33, dtype=np.uint8)
    rt, K = np.eye(4), np.array([[64.0, 0, 4], [0, 64.0, 2], [0, 0, 1]])
    ok = (w, 8 * w, w)
    cases = [("level -1", dict(level=-1), E_INVALID_ARGUMENT),
             ("level MAX", dict(level=native.MAX_LEVELS), E_INVALID_ARGUMENT),
             ("h 0", dict(h=0), E_SHAPE), ("w negative", dict(w=-w), E_SHAPE), ("w 0", dict(w=0), E_SHAPE),
             ("h negative", dict(h=-1), E_SHAPE),
             ("short gray stride", dict(strides=(w - 1, 8 * w, w)), E_SHAPE),
             ("short depth stride", dict(strides=(w, 8 * w - 1, w)), E_SHAPE),
             ("short output stride", dict(strides=(w, 8 * w, w - 1)), E_SHAPE)]
    cases += [(f"null {name}", dict(null=name), E_INVALID_ARGUMENT) for name in ("gray", "depth", "rt", "k", "out")]
    for what, change, status in cases:
        a = dict(level=0, w=w, h=h, strides=ok, null=None)
        a.update(change)
        got = _raw(g, d, rt, K, a["level"], a["w"], a["h"], out, strides=a["strides"], null=a["null"])
        assert got == status, (what, got)
        assert L.phovo_last_error(), what
        assert np.all(out == 33), what                               # a refusal writes nothing
        _good_call_still_works()
    assert native.MAX_LEVELS == wc.MAX_LEVELS
    # the last level itself is taken
    assert _raw(g, d, rt, K * np.array([[2.0 ** 15], [2.0 ** 15], [1.0]]), native.MAX_LEVELS - 1, w, h, out) == 0
    assert np.array_equal(out, g)


def test_a_device_index_past_the_last_is_a_hip_error():
    L = native.lib()
    w, h = 8, 4
    g, d, out = wc.gray_ramp(w, h), np.ones((h, w)), np.full((h, w), 33, dtype=np.uint8)
    n = L.phovo_device_count()
    assert n >= 1
    assert _raw(g, d, np.eye(4), np.eye(3), 0, w, h, out, device=n) == E_HIP
    assert L.phovo_last_error().decode().strip()
    assert np.all(out == 33)
    _good_call_still_works()


def test_warpImage_shape_mismatch_raises_and_views_are_converted():
    p = next(q for q in wc.small_problems() if q.name == "halving_32x16_L0")
    with pytest.raises(ValueError):
        odometry.warpImage(p.gray, p.depth[:, :-1], p.rt, p.K)
    with pytest.raises(ValueError):
        odometry.warpImage(p.gray[:-1], p.depth, p.rt, p.K)
    # non-contiguous views: every second column of wider planes, and a transposed Rt / K pair
    g2, d2 = np.zeros((p.h, 2 * p.w), dtype=np.uint8), np.zeros((p.h, 2 * p.w))
    g2[:, ::2], d2[:, ::2] = p.gray, p.depth
    gv, dv = g2[:, ::2], d2[:, ::2]
    rtv, kv = np.asfortranarray(p.rt), np.asfortranarray(p.K)
    assert not gv.flags.c_contiguous and not dv.flags.c_contiguous and not rtv.flags.c_contiguous
    assert np.array_equal(odometry.warpImage(gv, dv, rtv, kv), p.expected)
    # f32 depth: powers of two survive the conversion, so the image is that of the f64 copy -- the same closed form
    d32 = p.depth.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), p.depth)
    assert np.array_equal(odometry.warpImage(p.gray, d32, p.rt, p.K), p.expected)
    d = wc.sweep_draw(0)                                             # and with depths that do not survive it
    d32 = d["depth"].astype(np.float32)
    assert not np.array_equal(d32.astype(np.float64), d["depth"], equal_nan=True)
    exp = oracle.warp_image(d["gray"], d32.astype(np.float64), d["rt"], d["K"], d["level"])
    assert np.array_equal(odometry.warpImage(d["gray"], d32, d["rt"], d["K"], level=d["level"]), exp)
