"""ctypes loader for the reference build (oracle/_ref/libphovo_ref.so, built by oracle/Makefile.ref).

TEST INFRASTRUCTURE ONLY.  The library is the reference's own Analytic and BiObjective headers, compiled unmodified
against the stand-in headers of oracle/ref_standins/, behind the C surface of oracle/ref_driver.cpp.  It is what the
oracle, tests/biobjective_ref.py and the HIP kernels are compared with (tests/test_reference_build_cpu.py,
tests/test_gpu_reference_parity.py).

The reference tree is looked for where PHOVO_REFERENCE_DIR points (default /root/reference) and only read at build time.
A host without the tree builds nothing and uses a library that travelled with the working tree, if there is one.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_ref", "libphovo_ref.so")
_HEADERS = ("CPhotoconsistencyOdometry.h", "Matrix.h", "CPhotoconsistencyOdometryAnalytic.h",
            "CPhotoconsistencyOdometryBiObjective.h")


def reference_dir():
    return os.environ.get("PHOVO_REFERENCE_DIR", "/root/reference")


def tree_present():
    inc = os.path.join(reference_dir(), "phovo", "include")
    return all(os.path.isfile(os.path.join(inc, h)) for h in _HEADERS)


def library_path():
    return _SO


def build():
    """Tree absent: do nothing (returns None).  Tree present: run Makefile.ref; a failed compile raises."""
    if not tree_present():
        return None
    subprocess.check_call(["make", "-s", "-C", _HERE, "-f", "Makefile.ref", "PHOVO_REFERENCE_DIR=" + reference_dir()])
    return _SO


def available():
    return os.path.exists(_SO)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_SO)
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int)
        align = [C.POINTER(oracle.Config), dp, C.c_int, C.c_int, C.c_void_p, dp, C.c_void_p, dp, dp, dp, ip]
        L.phovo_ref_analytic_align.argtypes = align
        L.phovo_ref_biobjective_align.argtypes = align
        L.phovo_ref_analytic_optimize_levels.argtypes = [C.POINTER(oracle.Config), dp, C.POINTER(oracle.Level), dp, dp, ip]
        L.phovo_ref_eigen_pose.argtypes = [dp, dp]
        L.phovo_ref_eigen_pose.restype = None
        L.phovo_ref_warp_image.argtypes = [C.c_void_p, dp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def make_config(num_levels=None, blur=None, grad_scale=None, lam=None, max_iter=None, min_grad=None, min_depth=0.3,
                max_depth=5.0):
    """oracle.make_config without the oracle's library: the constructor defaults of the reference's classes, overridden
    per argument.  (The reference build then reads every per-level list from here; its own defaults never apply.)"""
    cfg = oracle.Config()
    cfg.num_levels = 5 if num_levels is None else int(num_levels)
    for l in range(oracle.MAX_LEVELS):
        cfg.blur_filter_size[l] = 0
        cfg.image_gradients_scaling_factor[l] = 0.0625
        cfg.lambda_optimization_step[l] = 1.0
        cfg.max_num_iterations[l] = {2: 5, 3: 20, 4: 50}.get(l, 0)
        cfg.min_gradient_norm[l] = 300.0
    for name, vals in (("blur_filter_size", blur), ("image_gradients_scaling_factor", grad_scale),
                       ("lambda_optimization_step", lam), ("max_num_iterations", max_iter),
                       ("min_gradient_norm", min_grad)):
        if vals is not None:
            arr = getattr(cfg, name)
            for i, v in enumerate(list(vals)[:oracle.MAX_LEVELS]):
                arr[i] = v
    cfg.min_depth, cfg.max_depth = float(min_depth), float(max_depth)
    return cfg


def _align(fn, cfg, K, gray0, depth0, gray1, depth1, init_state):
    g0, g1, d0 = _u8(gray0), _u8(gray1), _f64(depth0)
    d1 = None if depth1 is None else _f64(depth1)
    h, w = g0.shape
    assert g1.shape == (h, w) and d0.shape == (h, w) and (d1 is None or d1.shape == (h, w))
    state = np.zeros(6) if init_state is None else _f64(init_state).copy()
    rt = np.zeros(16)
    iters = (C.c_int * oracle.MAX_LEVELS)()
    Kf = _f64(K).reshape(9)
    rc = fn(C.byref(cfg), _dp(Kf), w, h, g0.ctypes.data, _dp(d0), g1.ctypes.data, None if d1 is None else _dp(d1),
            _dp(state), _dp(rt), iters)
    if rc != 0:
        raise RuntimeError(f"reference build failed with {rc}")
    return state, [iters[l] for l in range(cfg.num_levels)], rt.reshape(4, 4)


def analytic_align(cfg, K, gray0, depth0, gray1, depth1=None, init_state=None):
    """SetSourceFrame + SetTargetFrame + Optimize of the reference's Analytic class.
    Returns (state, iterations per level, 4x4 Rt)."""
    return _align(lib().phovo_ref_analytic_align, cfg, K, gray0, depth0, gray1, depth1, init_state)


def biobjective_align(cfg, K, gray0, depth0, gray1, depth1, init_state=None):
    """The same through the reference's BiObjective class."""
    return _align(lib().phovo_ref_biobjective_align, cfg, K, gray0, depth0, gray1, depth1, init_state)


def analytic_optimize(cfg, K, i0p, d0p, i1p, gxp, gyp, init_state=None):
    """Optimize of the Analytic class on prebuilt level planes (the arguments of oracle.optimize)."""
    arr, keep = oracle._levels_array(i0p, d0p, i1p, gxp, gyp)
    state = np.zeros(6) if init_state is None else _f64(init_state).copy()
    rt = np.zeros(16)
    iters = (C.c_int * oracle.MAX_LEVELS)()
    Kf = _f64(K).reshape(9)
    rc = lib().phovo_ref_analytic_optimize_levels(C.byref(cfg), _dp(Kf), arr, _dp(state), _dp(rt), iters)
    if rc != 0:
        raise RuntimeError(f"reference build failed with {rc}")
    return state, [iters[l] for l in range(cfg.num_levels)], rt.reshape(4, 4)


def eigen_pose(state):
    s = _f64(state)
    rt = np.zeros(16)
    lib().phovo_ref_eigen_pose(_dp(s), _dp(rt))
    return rt.reshape(4, 4)


def warp_image(gray_u8, depth, rt, K, level=0):
    g, d = _u8(gray_u8), _f64(depth)
    h, w = g.shape
    out = np.zeros_like(g)
    rtf, Kf = _f64(rt).reshape(16), _f64(K).reshape(9)
    rc = lib().phovo_ref_warp_image(g.ctypes.data, _dp(d), w, h, _dp(rtf), _dp(Kf), int(level), out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"reference build failed with {rc}")
    return out
