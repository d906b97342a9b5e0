"""Python host mirror of the reference's operator surface, over the C ABI.

`CPhotoconsistencyOdometryAnalytic` has the method names, argument meaning and call order of
phovo::Analytic::CPhotoconsistencyOdometryAnalytic<unsigned char,double>
(phovo/include/CPhotoconsistencyOdometryAnalytic.h:428-607); `AlignmentEngine` is the batched form
(one process per GPU, many independent frame pairs per launch).  Everything that computes runs in
libphovo_hip.so on the GPU; numpy only carries buffers across the boundary.
"""
import ctypes as C

import numpy as np

from . import native
from .native import check


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("intensity image must be 2-D (gray)")
    return a


def _f64img(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("depth image must be 2-D")
    return a


def gray_from_colour(pixels, channel_order="rgb"):
    """The project's one colour-to-gray rule, in numpy: (9797 R + 19234 G + 3737 B + 16384) >> 15 on u8 [..., 3] pixels --
    what apps/io/png_io.cpp applies to a colour PNG and the device ingest to RGB / BGR frames (integer arithmetic: all
    three agree exactly).  The coefficients are recalled from OpenCV's cvtColor, not checked against it."""
    p = np.asarray(pixels)
    if p.dtype != np.uint8 or p.shape[-1] != 3:
        raise ValueError("pixels must be uint8 [..., 3]")
    if channel_order not in ("rgb", "bgr"):
        raise ValueError('channel_order must be "rgb" or "bgr"')
    r, g, b = (p[..., i].astype(np.uint32) for i in ((0, 1, 2) if channel_order == "rgb" else (2, 1, 0)))
    return ((9797 * r + 19234 * g + 3737 * b + 16384) >> 15).astype(np.uint8)


def _depth_formats():
    """torch dtype -> PHOVO_IMAGE_* of a depth tensor; int16 storage is read as uint16."""
    import torch
    formats = {torch.float64: native.IMAGE_F64, torch.float32: native.IMAGE_F32, torch.float16: native.IMAGE_F16,
               torch.int16: native.IMAGE_U16}
    if hasattr(torch, "uint16"):
        formats[torch.uint16] = native.IMAGE_U16
    return formats


def _device_tensor(x, what, dtypes):
    """x as a torch tensor in device memory, without a copy: a torch tensor, or anything torch can view through
    __cuda_array_interface__ or DLPack.  A dtype outside `dtypes` and host memory are TypeErrors.  (torch is imported
    here, not with the package.)"""
    import torch
    if isinstance(x, torch.Tensor):
        t = x
    elif hasattr(x, "__cuda_array_interface__"):
        t = torch.as_tensor(x, device="cuda")
    elif hasattr(x, "__dlpack__") and hasattr(x, "__dlpack_device__"):
        t = torch.from_dlpack(x)
    else:
        raise TypeError(f"{what}: expected a torch tensor or an object with __cuda_array_interface__ / DLPack, got "
                        f"{type(x).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{what} must be one of {', '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if t.device.type == "cuda" and len(native.hip_runtimes_mapped()) > 1:
        raise RuntimeError("two HIP runtimes are loaded in this process (" + ", ".join(native.hip_runtimes_mapped()) + "): "
                           "torch was imported after libphovo_hip.so had loaded the system's.  Import torch before the "
                           "first use of phovo_amd so that both share one runtime")
    if t.device.type != "cuda":
        raise TypeError(f"{what} lives in host memory ({t.device}); upload_frames / Set*Frame take host arrays, the "
                        "*_device / *Device forms take device memory")
    return t


def _torch_stream(stream, device):
    """(torch stream object, raw hipStream_t handle) of `stream`: None = torch's current stream on `device`, a torch.cuda
    stream, or a raw handle as int."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(device)
    elif isinstance(stream, int):
        stream = torch.cuda.ExternalStream(stream, device=device)
    return stream, int(stream.cuda_stream)


def _device_images(gray, depth, channel_order, stream, device, batched):
    """phovo_device_image descriptors of gray ([F,H,W] u8 or [F,H,W,3] u8; without F unless batched) and depth ([F,H,W]
    float64 / float32 / float16 / uint16, or int16 storage read as uint16; None).  Row and frame strides are the
    tensors' own; only a pixel stride other than the element size (3 channels for colour) costs a .contiguous() copy, made
    on `stream`.  Returns (intensity, depth or None, tensors to keep alive, (F, H, W), raw stream handle)."""
    import torch
    resolved = []

    def the_stream():                        # (resolved after the tensors have been looked at: host memory is a TypeError
        if not resolved:                     # on a machine without a device too)
            resolved.extend(_torch_stream(stream, device))
        return resolved

    def packed(t, pixel_ok):
        if pixel_ok:
            return t
        with torch.cuda.stream(the_stream()[0]):
            return t.contiguous()

    g = _device_tensor(gray, "gray", (torch.uint8,))
    if not batched:
        g = g.unsqueeze(0)
    if g.ndim == 3:
        fmt = native.IMAGE_U8_GRAY
        g = packed(g, g.stride(2) == 1 or g.shape[2] == 1)
    elif g.ndim == 4 and g.shape[3] == 3:
        if channel_order not in ("rgb", "bgr"):
            raise ValueError('channel_order must be "rgb" or "bgr"')
        fmt = native.IMAGE_U8_RGB if channel_order == "rgb" else native.IMAGE_U8_BGR
        g = packed(g, g.stride(3) == 1 and (g.stride(2) == 3 or g.shape[2] == 1))
    else:
        raise ValueError("gray must be [frames, height, width] or [frames, height, width, 3]"
                         if batched else "gray must be [height, width] or [height, width, 3]")
    f, h, w = int(g.shape[0]), int(g.shape[1]), int(g.shape[2])
    gi = native.DeviceImage(g.data_ptr(), g.stride(1), g.stride(0), fmt, 0)
    keep = [g]
    di = None
    if depth is not None:
        formats = _depth_formats()
        d = _device_tensor(depth, "depth", tuple(formats))
        if not batched:
            d = d.unsqueeze(0)
        if d.ndim != 3 or tuple(d.shape) != (f, h, w):
            raise ValueError(f"depth shape {tuple(d.shape)} does not match gray's frames x height x width {(f, h, w)}")
        d = packed(d, d.stride(2) == 1 or w == 1)
        es = d.element_size()
        di = native.DeviceImage(d.data_ptr(), d.stride(1) * es, d.stride(0) * es, formats[d.dtype], 0)
        keep.append(d)
    return gi, di, keep, (f, h, w), the_stream()[1]


def warpImage(intensityImage, depthImage, Rt, intrinsicMatrix, level=0, device=0):
    """phovo::warpImage (phovo/include/CPhotoconsistencyOdometry.h:73-134) on the device: forward warp of the source
    intensities into the target view (depth > 0 gate, truncating cast, last raster writer wins, zeros elsewhere).
    Returns the warped u8 image instead of filling an output argument."""
    g, d = _u8(intensityImage), _f64img(depthImage)
    if g.shape != d.shape:
        raise ValueError("intensity and depth must have the same size")
    h, w = g.shape
    rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(16)
    k = np.ascontiguousarray(intrinsicMatrix, dtype=np.float64).reshape(9)
    out = np.empty((h, w), dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    check(native.lib().phovo_warp_image(int(device), g.ctypes.data, w, d.ctypes.data, w * 8, w, h,
                                        rt.ctypes.data_as(dp), k.ctypes.data_as(dp), int(level),
                                        out.ctypes.data, w), "warpImage")
    return out


class CPhotoconsistencyOdometryAnalytic:
    """One frame pair at a time; 1:1 with the reference class."""

    def __init__(self, device=0):
        self._lib = native.lib()
        self._h = C.c_void_p()
        check(self._lib.phovo_odometry_create(int(device), C.byref(self._h)), "phovo_odometry_create")
        self._device = int(device)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.phovo_odometry_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- configuration --------------------------------------------------------------------
    def ReadConfigurationFile(self, fileName):
        check(self._lib.phovo_odometry_read_configuration_file(self._h, str(fileName).encode()),
              "ReadConfigurationFile")

    def SetConfiguration(self, cfg):
        check(self._lib.phovo_odometry_set_config(self._h, C.byref(cfg)), "SetConfiguration")

    def SetExtensions(self, ext):
        """Not in the reference: plane storage / Huber weights (native.make_extensions)."""
        check(self._lib.phovo_odometry_set_extensions(self._h, C.byref(ext)), "SetExtensions")

    def SetLatencyForms(self, on=True):
        """Not in the reference: Optimize() may take the forms that finish soonest for one pair (last bits may then differ
        from the same pair aligned in a batch); default off."""
        check(self._lib.phovo_odometry_set_latency_forms(self._h, 1 if on else 0), "SetLatencyForms")

    def SetMinDepth(self, minD):
        check(self._lib.phovo_odometry_set_min_depth(self._h, float(minD)), "SetMinDepth")

    def SetMaxDepth(self, maxD):
        check(self._lib.phovo_odometry_set_max_depth(self._h, float(maxD)), "SetMaxDepth")

    def SetIntrinsicMatrix(self, intrinsicMatrix):
        k = np.ascontiguousarray(intrinsicMatrix, dtype=np.float64).reshape(9)
        check(self._lib.phovo_odometry_set_intrinsic_matrix(self._h, k.ctypes.data_as(C.POINTER(C.c_double))),
              "SetIntrinsicMatrix")

    # -- frames ---------------------------------------------------------------------------
    def SetSourceFrame(self, intensityImage, depthImage):
        g, d = _u8(intensityImage), _f64img(depthImage)
        if g.shape != d.shape:
            raise ValueError("intensity and depth sizes differ")
        h, w = g.shape
        check(self._lib.phovo_odometry_set_source_frame(self._h, g.ctypes.data, g.strides[0],
                                                        d.ctypes.data, d.strides[0], w, h), "SetSourceFrame")

    def SetTargetFrame(self, intensityImage, depthImage=None):
        g = _u8(intensityImage)
        h, w = g.shape
        d = _f64img(depthImage) if depthImage is not None else None
        check(self._lib.phovo_odometry_set_target_frame(
            self._h, g.ctypes.data, g.strides[0],
            d.ctypes.data if d is not None else None, d.strides[0] if d is not None else 0, w, h),
            "SetTargetFrame")

    def SetSourceFrameDevice(self, intensityImage, depthImage, depth_scale=1.0, channel_order="rgb", stream=None):
        """SetSourceFrame for images in device memory (torch tensors on this object's device, or anything torch views
        through __cuda_array_interface__ / DLPack): [H,W] u8 or [H,W,3] u8 with channel_order, depth [H,W] float64, or
        float32 / float16 / uint16 times depth_scale.  No host round trip and no synchronisation: the work is ordered
        behind `stream` (None: torch's current stream), and `stream` may overwrite the tensors right after the call."""
        if depthImage is None:
            raise ValueError("a source frame needs its depth")
        gi, di, _keep, (_, h, w), handle = _device_images(intensityImage, depthImage, channel_order, stream, self._device,
                                                          batched=False)
        check(self._lib.phovo_odometry_set_source_frame_device(self._h, C.byref(gi), C.byref(di), float(depth_scale), w, h,
                                                               handle), "SetSourceFrameDevice")

    def SetTargetFrameDevice(self, intensityImage, depthImage=None, depth_scale=1.0, channel_order="rgb", stream=None):
        """SetTargetFrame for images in device memory (see SetSourceFrameDevice); the depth is ignored except under the
        bi-objective."""
        gi, di, _keep, (_, h, w), handle = _device_images(intensityImage, depthImage, channel_order, stream, self._device,
                                                          batched=False)
        check(self._lib.phovo_odometry_set_target_frame_device(self._h, C.byref(gi), C.byref(di) if di is not None else None,
                                                               float(depth_scale), w, h, handle), "SetTargetFrameDevice")

    def SetInitialStateVector(self, initialStateVector):
        s = np.ascontiguousarray(initialStateVector, dtype=np.float64).reshape(6)
        check(self._lib.phovo_odometry_set_initial_state_vector(self._h, s.ctypes.data_as(C.POINTER(C.c_double))),
              "SetInitialStateVector")

    # -- optimisation ---------------------------------------------------------------------
    def Optimize(self):
        check(self._lib.phovo_odometry_optimize(self._h), "Optimize")

    def GetOptimalStateVector(self):
        s = np.zeros(6)
        check(self._lib.phovo_odometry_get_optimal_state_vector(self._h, s.ctypes.data_as(C.POINTER(C.c_double))),
              "GetOptimalStateVector")
        return s

    def GetOptimalRigidTransformationMatrix(self):
        rt = np.zeros(16)
        check(self._lib.phovo_odometry_get_optimal_rigid_transformation_matrix(
            self._h, rt.ctypes.data_as(C.POINTER(C.c_double))), "GetOptimalRigidTransformationMatrix")
        return rt.reshape(4, 4)

    def GetReport(self):
        rep = native.PairReport()
        check(self._lib.phovo_odometry_get_report(self._h, C.byref(rep)), "GetReport")
        return rep

    def GetPairSystem(self):
        """The Gauss-Newton system at the optimal state on the finest level the configuration optimises
        (native.PairSystem: information, gradient, cost, rows, flags); evaluated on demand after Optimize()."""
        ps = native.PairSystem()
        check(self._lib.phovo_odometry_get_pair_system(self._h, C.byref(ps)), "GetPairSystem")
        return ps

    def GetSampledSystem(self):
        """The Gauss-Newton system of the sampled aligners (bilinear sampling: dim 6; the affine-illumination objective:
        dim 8, at the (alpha, beta) of the last Optimize()) at the optimal state on the finest level the configuration
        optimises (native.SampledSystem); evaluated on demand after Optimize()."""
        ss = native.SampledSystem()
        check(self._lib.phovo_odometry_get_sampled_system(self._h, C.byref(ss)), "GetSampledSystem")
        return ss

    def LastOptimizeMilliseconds(self):
        ms = C.c_double()
        check(self._lib.phovo_odometry_last_optimize_ms(self._h, C.byref(ms)), "LastOptimizeMilliseconds")
        return ms.value


class CPhotoconsistencyOdometryBiObjective(CPhotoconsistencyOdometryAnalytic):
    """One frame pair at a time; 1:1 with the reference's CPhotoconsistencyOdometryBiObjective (photometric and depth
    error together).  The target frame keeps its depth: SetTargetFrame requires it."""

    def __init__(self, device=0):
        super().__init__(device)
        check(self._lib.phovo_odometry_set_objective(self._h, native.OBJECTIVE_BIOBJECTIVE), "SetObjective")

    def SetTargetFrame(self, intensityImage, depthImage):
        if depthImage is None:
            raise ValueError("the bi-objective needs the target's depth")
        super().SetTargetFrame(intensityImage, depthImage)

    def SetTargetFrameDevice(self, intensityImage, depthImage, depth_scale=1.0, channel_order="rgb", stream=None):
        if depthImage is None:
            raise ValueError("the bi-objective needs the target's depth")
        super().SetTargetFrameDevice(intensityImage, depthImage, depth_scale, channel_order, stream)

    def GetObjectiveSystem(self):
        """native.PairSystem of the 2N-row system at the optimal state on the finest level the configuration optimises
        (rows: contributing source pixels; cost: r^T r over all 2N residuals); evaluated on demand after Optimize()."""
        ps = native.PairSystem()
        check(self._lib.phovo_odometry_get_objective_system(self._h, C.byref(ps)), "GetObjectiveSystem")
        return ps


class CPhotoconsistencyOdometryCeres(CPhotoconsistencyOdometryAnalytic):
    """One frame pair at a time; 1:1 with the reference's phovo::Ceres::CPhotoconsistencyOdometryCeres (bilinear samples,
    exact warp Jacobian, Levenberg-Marquardt trust region per level; hand-derived derivatives in HIP, no Ceres).
    ReadConfigurationFile reads the Ceres keys.  Optimize() does not print; GetSolverReport() returns what it did."""

    def __init__(self, device=0):
        super().__init__(device)
        check(self._lib.phovo_odometry_set_objective(self._h, native.OBJECTIVE_TRUST_REGION), "SetObjective")

    def SetTrustRegionOptions(self, opt):
        check(self._lib.phovo_odometry_set_trust_region_options(self._h, C.byref(opt)), "SetTrustRegionOptions")

    def GetTrustRegionOptions(self):
        opt = native.TrustRegionOptions()
        check(self._lib.phovo_odometry_get_trust_region_options(self._h, C.byref(opt)), "GetTrustRegionOptions")
        return opt

    def GetSolverReport(self):
        """native.TrustRegionReport of the last Optimize(): per level steps, accepted, termination, rows, costs, radius."""
        rep = native.TrustRegionReport()
        check(self._lib.phovo_odometry_get_trust_region_report(self._h, C.byref(rep)), "GetSolverReport")
        return rep

    def GetObjectiveSystem(self):
        """native.PairSystem at the optimal state on the finest level the configuration optimises: J^T J, J^T r, rows (owned
        targets) and cost = r^T r, which is twice Ceres's cost and twice the solver report's final_cost; evaluated on demand
        after Optimize()."""
        ps = native.PairSystem()
        check(self._lib.phovo_odometry_get_objective_system(self._h, C.byref(ps)), "GetObjectiveSystem")
        return ps


class CPhotoconsistencyOdometryAffine(CPhotoconsistencyOdometryAnalytic):
    """One frame pair at a time; not in the reference: the photometric objective with a per-pair gain and offset estimated
    jointly with the pose (native.OBJECTIVE_PHOTOMETRIC_AFFINE: bilinear samples, exact warp Jacobian, residual
    I1 - (1 + alpha) I0 - beta).  Reads the analytic yml files; extensions and GetPairSystem() are refused
    (PHOVO_E_UNSUPPORTED); GetSampledSystem() returns the 8 x 8 system.  GetIllumination() returns what Optimize() found."""

    def __init__(self, device=0):
        super().__init__(device)
        check(self._lib.phovo_odometry_set_objective(self._h, native.OBJECTIVE_PHOTOMETRIC_AFFINE), "SetObjective")

    def GetIllumination(self):
        """(alpha, beta) of the last Optimize(): the target's intensities are modelled as (1 + alpha) I0 + beta."""
        ab = np.zeros(2)
        check(self._lib.phovo_odometry_get_illumination(self._h, ab.ctypes.data_as(C.POINTER(C.c_double))),
              "GetIllumination")
        return ab


class CPhotoconsistencyOdometryGeometric(CPhotoconsistencyOdometryAnalytic):
    """One frame pair at a time; not in the reference: intensity and depth rows together on the bilinear samples
    (native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC: residuals I1 - I0 and sigma (D1 - Z'), exact warp Jacobian).  The
    target frame's depth is used: SetTargetFrame requires it.  Reads the analytic yml files and their two optional keys;
    extensions, GetPairSystem() and GetSampledSystem() are refused (PHOVO_E_UNSUPPORTED); GetGeometricSystem() returns this
    objective's system with the photometric and the depth block apart."""

    def __init__(self, device=0):
        super().__init__(device)
        check(self._lib.phovo_odometry_set_objective(self._h, native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC), "SetObjective")

    def SetTargetFrame(self, intensityImage, depthImage):
        if depthImage is None:
            raise ValueError("the photometric-geometric objective needs the target's depth")
        super().SetTargetFrame(intensityImage, depthImage)

    def SetTargetFrameDevice(self, intensityImage, depthImage, depth_scale=1.0, channel_order="rgb", stream=None):
        if depthImage is None:
            raise ValueError("the photometric-geometric objective needs the target's depth")
        super().SetTargetFrameDevice(intensityImage, depthImage, depth_scale, channel_order, stream)

    def SetGeometricOptions(self, opt):
        """native.GeometricOptions (native.make_geometric_options / read_geometric_file)."""
        check(self._lib.phovo_odometry_set_geometric_options(self._h, C.byref(opt)), "SetGeometricOptions")

    def GetGeometricOptions(self):
        opt = native.GeometricOptions()
        check(self._lib.phovo_odometry_get_geometric_options(self._h, C.byref(opt)), "GetGeometricOptions")
        return opt

    def GetGeometricReport(self):
        """native.GeometricReport of the last Optimize(): per level depth_rows, photometric_cost, depth_cost."""
        rep = native.GeometricReport()
        check(self._lib.phovo_odometry_get_geometric_report(self._h, C.byref(rep)), "GetGeometricReport")
        return rep

    def GetGeometricSystem(self):
        """native.GeometricSystem at the optimal state on the finest level the configuration optimises: the photometric and
        the depth block of the Gauss-Newton system apart, and their sum; evaluated on demand after Optimize()."""
        gs = native.GeometricSystem()
        check(self._lib.phovo_odometry_get_geometric_system(self._h, C.byref(gs)), "GetGeometricSystem")
        return gs


class _PosePrior:
    """The Gaussian pose prior of the two inverse-compositional classes (phovo_hip.h, phovo_prior_options)."""

    def SetPosePrior(self, state, information):
        """The prior of every later Optimize() until ClearPosePrior(): state[6] the prior pose (x, y, z, yaw, pitch, roll),
        information[6, 6] symmetric, in the twist order (nu, omega) of GetInverseSystem(); its upper triangle is read."""
        st = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
        info = np.ascontiguousarray(information, dtype=np.float64).reshape(-1)
        if st.size != 6 or info.size != 36:
            raise ValueError("SetPosePrior: state must have 6 entries and information 6 x 6")
        dp = C.POINTER(C.c_double)
        check(self._lib.phovo_odometry_set_pose_prior(self._h, st.ctypes.data_as(dp), info.ctypes.data_as(dp)), "SetPosePrior")

    def ClearPosePrior(self):
        check(self._lib.phovo_odometry_clear_pose_prior(self._h), "ClearPosePrior")

    def SetPriorOptions(self, opt):
        """native.PriorOptions (native.make_prior_options)."""
        check(self._lib.phovo_odometry_set_prior_options(self._h, C.byref(opt)), "SetPriorOptions")

    def GetPriorOptions(self):
        opt = native.PriorOptions()
        check(self._lib.phovo_odometry_get_prior_options(self._h, C.byref(opt)), "GetPriorOptions")
        return opt

    def GetPriorReport(self):
        """native.PriorReport of the last Optimize(), which carried a prior: e = Log(T_p^-1 T) and e^T Lambda e."""
        rep = native.PriorReport()
        check(self._lib.phovo_odometry_get_prior_report(self._h, C.byref(rep)), "GetPriorReport")
        return rep


class CPhotoconsistencyOdometryInverse(_PosePrior, CPhotoconsistencyOdometryAnalytic):
    """One frame pair at a time; not in the reference: the photometric residual aligned inverse-compositionally
    (native.OBJECTIVE_INVERSE_COMPOSITIONAL: bilinear samples of the target, the Jacobian from the source frame's own
    gradient, the step composed on SE(3)).  SetSourceFrame also builds the source's gradient planes.  Reads
    the analytic yml files; extensions and the Euler-basis Get...System() calls are refused (PHOVO_E_UNSUPPORTED);
    GetInverseSystem() returns this objective's system in the twist basis."""

    def __init__(self, device=0):
        super().__init__(device)
        check(self._lib.phovo_odometry_set_objective(self._h, native.OBJECTIVE_INVERSE_COMPOSITIONAL), "SetObjective")

    def GetInverseSystem(self):
        """native.PairSystem at the optimal state on the finest level the configuration optimises, in the twist basis
        (nu, omega) of a right-hand perturbation T Exp(xi) in the source camera's frame: sum J J^T, sum J r, rows and
        cost = sum r^2; evaluated on demand after Optimize()."""
        ps = native.PairSystem()
        check(self._lib.phovo_odometry_get_inverse_system(self._h, C.byref(ps)), "GetInverseSystem")
        return ps


class CPhotoconsistencyOdometryRobust(_PosePrior, CPhotoconsistencyOdometryAnalytic):
    """One frame pair at a time; not in the reference: the inverse-compositional aligner under a Huber weight whose
    threshold is scale_factor times the median of |r| over the pair's own rows (native.OBJECTIVE_INVERSE_ROBUST, DESIGN.md
    §22).  SetSourceFrame also builds the source's gradient planes.  Reads the analytic yml files; extensions and every
    Get...System() call are refused (PHOVO_E_UNSUPPORTED)."""

    def __init__(self, device=0):
        super().__init__(device)
        check(self._lib.phovo_odometry_set_objective(self._h, native.OBJECTIVE_INVERSE_ROBUST), "SetObjective")

    def SetRobustOptions(self, opt):
        """native.RobustOptions (native.make_robust_options)."""
        check(self._lib.phovo_odometry_set_robust_options(self._h, C.byref(opt)), "SetRobustOptions")

    def GetRobustOptions(self):
        opt = native.RobustOptions()
        check(self._lib.phovo_odometry_get_robust_options(self._h, C.byref(opt)), "GetRobustOptions")
        return opt

    def GetRobustSystem(self):
        """native.RobustSystem at the optimal state on the finest level the configuration optimises, with the median rule
        taken at that state: sum w J J^T, sum w J r in the twist basis of GetInverseSystem(), the three costs, delta, the
        median, rows and outliers; evaluated on demand after Optimize()."""
        rs = native.RobustSystem()
        check(self._lib.phovo_odometry_get_robust_system(self._h, C.byref(rs)), "GetRobustSystem")
        return rs

    def GetRobustReport(self):
        """native.RobustReport of the last Optimize(): per level the delta and the outliers of the last system."""
        rep = native.RobustReport()
        check(self._lib.phovo_odometry_get_robust_report(self._h, C.byref(rep)), "GetRobustReport")
        return rep


class CPhotoconsistencyOdometrySemiDense(CPhotoconsistencyOdometryAnalytic):
    """One frame pair at a time; not in the reference: the inverse-compositional aligner on the source pixels selected
    once per level by depth and gradient magnitude (native.OBJECTIVE_INVERSE_SEMIDENSE).  SetSourceFrame
    also builds the source's gradient planes.  Reads the analytic yml files and their optional key
    `min_pixel_gradient (at each level)`; extensions and every Get...System() call are refused (PHOVO_E_UNSUPPORTED)."""

    def __init__(self, device=0):
        super().__init__(device)
        check(self._lib.phovo_odometry_set_objective(self._h, native.OBJECTIVE_INVERSE_SEMIDENSE), "SetObjective")

    def SetSemiDenseOptions(self, opt):
        """native.SemiDenseOptions (native.make_semidense_options)."""
        check(self._lib.phovo_odometry_set_semidense_options(self._h, C.byref(opt)), "SetSemiDenseOptions")

    def GetSemiDenseOptions(self):
        opt = native.SemiDenseOptions()
        check(self._lib.phovo_odometry_get_semidense_options(self._h, C.byref(opt)), "GetSemiDenseOptions")
        return opt

    def GetSemiDenseReport(self):
        """native.SemiDenseReport of the last Optimize(): per level the number of selected pixels."""
        rep = native.SemiDenseReport()
        check(self._lib.phovo_odometry_get_semidense_report(self._h, C.byref(rep)), "GetSemiDenseReport")
        return rep


# phovo_semidense_report as a numpy record
SEMIDENSE_REPORT_DTYPE = np.dtype([("selected", "<i4", (native.MAX_LEVELS,))])
assert SEMIDENSE_REPORT_DTYPE.itemsize == C.sizeof(native.SemiDenseReport)


def semidense_thresholds(engine, frame, fraction, min_depth=None, max_depth=None):
    """Per level the tau_L that keeps about `fraction` of the depth-valid pixels of `frame` (0 < fraction <= 1) under
    native.OBJECTIVE_INVERSE_SEMIDENSE: the (1 - fraction) quantile of the gradient magnitude over the pixels with
    min_depth < D < max_depth, on the planes read back from the pool, moved to the middle of the gap between the two
    samples around it.  The depth range is the one the engine was given through set_depth_range (0.3 ... 5.0 without such a
    call), unless passed here.  Host-side only; a list of native.MAX_LEVELS values
    (0 for levels the pool does not hold, and where no pixel is depth-valid) for native.make_semidense_options."""
    if not 0.0 < fraction <= 1.0:
        raise ValueError("semidense_thresholds: fraction must lie in (0, 1]")
    # the depth gate of the selection is the engine's: what set_depth_range was given, else the library's default
    lo, hi = getattr(engine, "depth_range", (0.3, 5.0))
    min_depth = lo if min_depth is None else min_depth
    max_depth = hi if max_depth is None else max_depth
    taus = [0.0] * native.MAX_LEVELS
    for level in range(engine.get_config().num_levels):
        if not engine._lib.phovo_engine_level_is_stored(engine._h, level):
            continue
        _, d, gx, gy = engine.get_level_planes(frame, level)
        with np.errstate(invalid="ignore"):
            ok = (d > min_depth) & (d < max_depth)
        g = np.sqrt(gx[ok] * gx[ok] + gy[ok] * gy[ok])
        g = g[np.isfinite(g)]
        if g.size and fraction < 1.0:
            taus[level] = _between_samples(g, float(np.quantile(g, 1.0 - fraction)))
    return taus


def _between_samples(g, q):
    """q moved to the middle of the gap between the samples next to it (the largest <= q, the smallest > q), so that no
    pixel sits on the threshold and rounding cannot decide a pixel's selection; q itself where no sample lies above it."""
    above = g[g > q * (1.0 + 1e-9)]                  # (samples within rounding of q count as q)
    below = g[g <= q * (1.0 + 1e-9)]
    return 0.5 * (float(below.max()) + float(above.min())) if above.size and below.size else q


# phovo_robust_report as a numpy record: one row of per-level fields per pair
ROBUST_REPORT_DTYPE = np.dtype({"names": ["delta", "outliers"], "formats": [("<f8", (native.MAX_LEVELS,)), ("<i4", (native.MAX_LEVELS,))],
                                "offsets": [native.RobustReport.delta.offset, native.RobustReport.outliers.offset],
                                "itemsize": C.sizeof(native.RobustReport)})

# phovo_prior_report as a numpy record
PRIOR_REPORT_DTYPE = np.dtype([("error", "<f8", (6,)), ("prior_cost", "<f8")])
assert PRIOR_REPORT_DTYPE.itemsize == C.sizeof(native.PriorReport)

# phovo_geometric_report as a numpy record: one row of per-level fields per pair
GEOMETRIC_REPORT_DTYPE = np.dtype([("depth_rows", "<i4", (native.MAX_LEVELS,)),
                                   ("photometric_cost", "<f8", (native.MAX_LEVELS,)),
                                   ("depth_cost", "<f8", (native.MAX_LEVELS,))])
assert GEOMETRIC_REPORT_DTYPE.itemsize == C.sizeof(native.GeometricReport)

# phovo_trust_region_report as a numpy record: one row of per-level fields per pair
TRUST_REGION_REPORT_DTYPE = np.dtype([("steps", "<i4", (native.MAX_LEVELS,)), ("accepted", "<i4", (native.MAX_LEVELS,)),
                                      ("termination", "<i4", (native.MAX_LEVELS,)), ("rows", "<i4", (native.MAX_LEVELS,)),
                                      ("initial_cost", "<f8", (native.MAX_LEVELS,)),
                                      ("final_cost", "<f8", (native.MAX_LEVELS,)),
                                      ("final_radius", "<f8", (native.MAX_LEVELS,)),
                                      ("jacobi_scaling", "<f8", (native.MAX_LEVELS, 6))])
_TR_LEVEL_DTYPE = np.dtype([("steps", "<i4"), ("accepted", "<i4"), ("termination", "<i4"), ("rows", "<i4"),
                            ("initial_cost", "<f8"), ("final_cost", "<f8"), ("final_radius", "<f8"),
                            ("jacobi_scaling", "<f8", (6,))])
assert _TR_LEVEL_DTYPE.itemsize * native.MAX_LEVELS == C.sizeof(native.TrustRegionReport)


# phovo_pair_system as a numpy record (352 bytes, the layout of native.PairSystem): evaluate_pairs fills an array of
# these in place and returns column views, with no per-record Python work
PAIR_SYSTEM_DTYPE = np.dtype([("information", "<f8", (36,)), ("gradient", "<f8", (6,)), ("cost", "<f8"),
                              ("rows", "<i4"), ("flags", "<u4")])
assert PAIR_SYSTEM_DTYPE.itemsize == C.sizeof(native.PairSystem)


# phovo_sampled_system as a numpy record (the layout of native.SampledSystem): evaluate_sampled_pairs fills an array of these
SAMPLED_SYSTEM_DTYPE = np.dtype([("information", "<f8", (native.SYSTEM_MAX_DIM * native.SYSTEM_MAX_DIM,)),
                                 ("gradient", "<f8", (native.SYSTEM_MAX_DIM,)), ("cost", "<f8"), ("rows", "<i4"),
                                 ("flags", "<u4"), ("dim", "<i4"), ("reserved", "<i4")])
assert SAMPLED_SYSTEM_DTYPE.itemsize == C.sizeof(native.SampledSystem)


# phovo_geometric_system as a numpy record (the layout of native.GeometricSystem): evaluate_geometric_pairs returns an array
# of these
GEOMETRIC_SYSTEM_DTYPE = np.dtype([("information", "<f8", (36,)), ("gradient", "<f8", (6,)),
                                   ("photometric_information", "<f8", (36,)), ("photometric_gradient", "<f8", (6,)),
                                   ("depth_information", "<f8", (36,)), ("depth_gradient", "<f8", (6,)),
                                   ("photometric_cost", "<f8"), ("depth_cost", "<f8"), ("rows", "<i4"),
                                   ("depth_rows", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
assert GEOMETRIC_SYSTEM_DTYPE.itemsize == C.sizeof(native.GeometricSystem)


# phovo_robust_system as a numpy record (the layout of native.RobustSystem): evaluate_robust_pairs fills an array of these
ROBUST_SYSTEM_DTYPE = np.dtype([("information", "<f8", (36,)), ("gradient", "<f8", (6,)), ("cost", "<f8"),
                                ("huber_cost", "<f8"), ("squared_cost", "<f8"), ("delta", "<f8"), ("median", "<f8"),
                                ("rows", "<i4"), ("outliers", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
assert ROBUST_SYSTEM_DTYPE.itemsize == C.sizeof(native.RobustSystem)


class AlignmentEngine:
    """Batched alignment: a pool of frames resident in HBM, pairs aligned one launch per level."""

    def __init__(self, device=0):
        self._lib = native.lib()
        self._h = C.c_void_p()
        check(self._lib.phovo_engine_create(int(device), C.byref(self._h)), "phovo_engine_create")
        self._device = int(device)
        self.n_frames = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.phovo_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_config(self, cfg):
        check(self._lib.phovo_engine_set_config(self._h, C.byref(cfg)), "phovo_engine_set_config")

    def read_configuration_file(self, path):
        self.set_extensions(native.read_extensions_file(path))
        self.set_config(native.read_config_file(path))

    def set_extensions(self, ext):
        """Changing plane_storage drops the frame pool; so does changing `sampling` on fp16 planes (their bilinear tap
        records are added or removed).  The call succeeds, and the next align_pairs raises PhovoError with status
        E_NOT_READY until reserve_frames and the uploads have been repeated.  Any other change keeps the frames."""
        check(self._lib.phovo_engine_set_extensions(self._h, C.byref(ext)), "phovo_engine_set_extensions")

    def get_extensions(self):
        ext = native.Extensions()
        check(self._lib.phovo_engine_get_extensions(self._h, C.byref(ext)), "phovo_engine_get_extensions")
        return ext

    def get_config(self):
        cfg = native.Config()
        check(self._lib.phovo_engine_get_config(self._h, C.byref(cfg)), "phovo_engine_get_config")
        return cfg

    def set_intrinsic_matrix(self, K):
        k = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        check(self._lib.phovo_engine_set_intrinsic_matrix(self._h, k.ctypes.data_as(C.POINTER(C.c_double))),
              "phovo_engine_set_intrinsic_matrix")

    def set_depth_range(self, min_depth, max_depth):
        check(self._lib.phovo_engine_set_depth_range(self._h, float(min_depth), float(max_depth)),
              "phovo_engine_set_depth_range")
        self.depth_range = (float(min_depth), float(max_depth))      # (the library has no getter; semidense_thresholds reads it)

    def set_build_all_levels(self, on):
        check(self._lib.phovo_engine_set_build_all_levels(self._h, int(bool(on))), "phovo_engine_set_build_all_levels")

    def set_wide_policy(self, policy):
        """0 automatic, 1 wide form wherever possible, -1 persistent form only."""
        check(self._lib.phovo_engine_set_wide_policy(self._h, int(policy)), "phovo_engine_set_wide_policy")

    def set_level_fusion(self, mode):
        """native.FUSION_AUTO (default): consecutive levels that fit the 512-thread scatter kernel are ONE launch when a
        gradient threshold makes their iteration counts data-dependent; FUSION_OFF: one launch per level; FUSION_SPLIT: one
        launch per level in the fused launch's geometry (bit-identical to AUTO)."""
        check(self._lib.phovo_engine_set_level_fusion(self._h, int(mode)), "phovo_engine_set_level_fusion")

    def set_batch_invariant(self, on=True):
        """Every batch, whatever its size, takes the same kernels and geometries: a pair's result does not depend on how
        many other pairs are aligned with it (what the sequence drivers set, so that a sequence cut into shards of any
        sizes gives bit-identical poses)."""
        check(self._lib.phovo_engine_set_batch_invariant(self._h, int(bool(on))), "phovo_engine_set_batch_invariant")

    def set_latency_forms(self, on=True):
        """A handful of pairs may take the forms that finish soonest also on levels of <= ~39 k pixels (last bits may then
        differ from the batch forms); default off: one arithmetic per pair on those levels."""
        check(self._lib.phovo_engine_set_latency_forms(self._h, 1 if on else 0), "phovo_engine_set_latency_forms")

    def set_slide_policy(self, policy):
        """0 automatic (sliding-window kernel on levels whose owner map exceeds LDS), -1 exact kernel only."""
        check(self._lib.phovo_engine_set_slide_policy(self._h, int(policy)), "phovo_engine_set_slide_policy")

    def level_uses_wide(self, level, n_pairs):
        return bool(self._lib.phovo_engine_level_uses_wide(self._h, int(level), int(n_pairs)))

    def reserve_frames(self, n_frames, width, height):
        check(self._lib.phovo_engine_reserve_frames(self._h, int(n_frames), int(width), int(height)),
              "phovo_engine_reserve_frames")
        self.n_frames = int(n_frames)

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        check(self._lib.phovo_engine_level_size(self._h, int(level), C.byref(w), C.byref(h)), "phovo_engine_level_size")
        return w.value, h.value

    def level_is_stored(self, level):
        return bool(self._lib.phovo_engine_level_is_stored(self._h, int(level)))

    def upload_frame(self, frame, gray, depth=None, roles=native.ROLE_BOTH):
        g = _u8(gray)
        d = _f64img(depth) if depth is not None else None
        check(self._lib.phovo_engine_upload_frame(
            self._h, int(frame), int(roles), g.ctypes.data, g.strides[0],
            d.ctypes.data if d is not None else None, d.strides[0] if d is not None else 0),
            "phovo_engine_upload_frame")

    def upload_frame_u16(self, frame, gray, depth_u16, depth_scale, roles=native.ROLE_BOTH):
        g = _u8(gray)
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        check(self._lib.phovo_engine_upload_frame_u16(
            self._h, int(frame), int(roles), g.ctypes.data, g.strides[0], d.ctypes.data, d.strides[0],
            float(depth_scale)), "phovo_engine_upload_frame_u16")

    def upload_frames(self, first_frame, gray, depth=None, depth_scale=None, roles=native.ROLE_BOTH):
        """Batched upload of gray [F,H,W] u8 with depth [F,H,W] fp64 (metres) or u16 (with depth_scale)."""
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        if g.ndim != 3:
            raise ValueError("gray must be [frames, height, width]")
        if depth is None:
            check(self._lib.phovo_engine_upload_frames(self._h, int(first_frame), g.shape[0], int(roles), g.ctypes.data,
                                                       g.strides[1], g.strides[0], None, 0, 0), "phovo_engine_upload_frames")
        elif depth_scale is None:
            d = np.ascontiguousarray(depth, dtype=np.float64)
            check(self._lib.phovo_engine_upload_frames(self._h, int(first_frame), g.shape[0], int(roles), g.ctypes.data,
                                                       g.strides[1], g.strides[0], d.ctypes.data, d.strides[1], d.strides[0]),
                  "phovo_engine_upload_frames")
        else:
            d = np.ascontiguousarray(depth, dtype=np.uint16)
            check(self._lib.phovo_engine_upload_frames_u16(self._h, int(first_frame), g.shape[0], int(roles), g.ctypes.data,
                                                           g.strides[1], g.strides[0], d.ctypes.data, d.strides[1], d.strides[0],
                                                           float(depth_scale)), "phovo_engine_upload_frames_u16")

    def upload_frames_device(self, first_frame, gray, depth=None, depth_scale=1.0, roles=native.ROLE_BOTH, stream=None,
                             channel_order="rgb"):
        """upload_frames for frames that already live in device memory (phovo_engine_upload_frames_device): no host round
        trip, no host synchronisation, and exactly the planes the host upload of the same pixel values gives.
          gray   [F,H,W] uint8, or [F,H,W,3] uint8 with channel_order "rgb" | "bgr" (gray_from_colour's integer rule)
          depth  [F,H,W] float64 (metres; depth_scale 1), or float32 / float16 / uint16: (double)value * depth_scale.
                 int16 storage is accepted and read as uint16 (for torch builds without a uint16 dtype).
        Both are torch tensors on the engine's device, or objects torch can view without a copy (__cuda_array_interface__,
        DLPack).  Row and frame strides are passed through as they are (slices of larger tensors cost nothing); only a
        pixel stride other than the element size makes a .contiguous() copy.  A CPU tensor or numpy array is a TypeError.
        `stream`: the torch.cuda stream (or raw handle) the tensors were produced on, None = torch's current stream of
        the engine's device.  The engine reads the tensors behind what that stream has queued, and the stream waits for
        the read: the caller may overwrite or drop the tensors on that stream right after this returns.  Later align /
        evaluate / plane calls are ordered behind the ingest.
        In a process that uses torch, import it before the first use of this package (one HIP runtime for both:
        native.hip_runtimes_mapped); a RuntimeError says so otherwise."""
        gi, di, _keep, (f, h, w), handle = _device_images(gray, depth, channel_order, stream, self._device, batched=True)
        if self.n_frames:
            pw, ph = self.level_size(0)
            if (w, h) != (pw, ph):
                raise ValueError(f"frames are {w}x{h}, the pool was reserved for {pw}x{ph}")
        check(self._lib.phovo_engine_upload_frames_device(self._h, int(first_frame), f, int(roles), C.byref(gi),
                                                          C.byref(di) if di is not None else None, float(depth_scale),
                                                          handle), "phovo_engine_upload_frames_device")

    def last_ingest(self):
        """What the last upload_frames_device launched: dict(chunks, wide_launches, scalar_launches)."""
        rec = native.IngestRecord()
        check(self._lib.phovo_engine_last_ingest(self._h, C.byref(rec)), "phovo_engine_last_ingest")
        return dict(chunks=rec.chunks, wide_launches=rec.wide_launches, scalar_launches=rec.scalar_launches)

    def set_objective(self, objective):
        """native.OBJECTIVE_PHOTOMETRIC (default) or native.OBJECTIVE_BIOBJECTIVE; a change drops the frame pool."""
        check(self._lib.phovo_engine_set_objective(self._h, int(objective)), "phovo_engine_set_objective")

    def get_objective(self):
        v = C.c_int()
        check(self._lib.phovo_engine_get_objective(self._h, C.byref(v)), "phovo_engine_get_objective")
        return v.value

    def set_trust_region_options(self, opt):
        """native.TrustRegionOptions (native.make_trust_region_options / read_trust_region_file)."""
        check(self._lib.phovo_engine_set_trust_region_options(self._h, C.byref(opt)),
              "phovo_engine_set_trust_region_options")

    def get_trust_region_options(self):
        opt = native.TrustRegionOptions()
        check(self._lib.phovo_engine_get_trust_region_options(self._h, C.byref(opt)),
              "phovo_engine_get_trust_region_options")
        return opt

    def read_trust_region_file(self, path):
        """A Ceres-method yml: its config and solver options."""
        cfg, opt = native.read_trust_region_file(path)
        self.set_trust_region_options(opt)
        self.set_config(cfg)

    def fetch_illumination(self, n_pairs):
        """(alpha, beta) of every pair of the last enqueue, which ran under native.OBJECTIVE_PHOTOMETRIC_AFFINE: an
        (n_pairs, 2) float64 array."""
        out = np.zeros((int(n_pairs), 2), dtype=np.float64)
        check(self._lib.phovo_engine_fetch_illumination(self._h, int(n_pairs), out.ctypes.data),
              "phovo_engine_fetch_illumination")
        return out

    def set_geometric_options(self, opt):
        """native.GeometricOptions (native.make_geometric_options / read_geometric_file)."""
        check(self._lib.phovo_engine_set_geometric_options(self._h, C.byref(opt)), "phovo_engine_set_geometric_options")

    def get_geometric_options(self):
        opt = native.GeometricOptions()
        check(self._lib.phovo_engine_get_geometric_options(self._h, C.byref(opt)), "phovo_engine_get_geometric_options")
        return opt

    def fetch_geometric_reports(self, n_pairs):
        """The records of the last enqueue's pairs, which ran under native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC, as one
        structured numpy array of GEOMETRIC_REPORT_DTYPE: out["depth_rows"][p, L], out["photometric_cost"][p, L],
        out["depth_cost"][p, L]."""
        out = np.zeros(int(n_pairs), dtype=GEOMETRIC_REPORT_DTYPE)
        check(self._lib.phovo_engine_fetch_geometric_reports(self._h, int(n_pairs), out.ctypes.data),
              "phovo_engine_fetch_geometric_reports")
        return out

    def set_robust_options(self, opt):
        """native.RobustOptions (native.make_robust_options)."""
        check(self._lib.phovo_engine_set_robust_options(self._h, C.byref(opt)), "phovo_engine_set_robust_options")

    def get_robust_options(self):
        opt = native.RobustOptions()
        check(self._lib.phovo_engine_get_robust_options(self._h, C.byref(opt)), "phovo_engine_get_robust_options")
        return opt

    def set_semidense_options(self, opt):
        """native.SemiDenseOptions (native.make_semidense_options)."""
        check(self._lib.phovo_engine_set_semidense_options(self._h, C.byref(opt)), "phovo_engine_set_semidense_options")

    def get_semidense_options(self):
        opt = native.SemiDenseOptions()
        check(self._lib.phovo_engine_get_semidense_options(self._h, C.byref(opt)), "phovo_engine_get_semidense_options")
        return opt

    def fetch_semidense_reports(self, n_pairs):
        """The records of the last enqueue's pairs, which ran under native.OBJECTIVE_INVERSE_SEMIDENSE, as one structured
        numpy array of SEMIDENSE_REPORT_DTYPE: out["selected"][p, L]."""
        out = np.zeros(int(n_pairs), dtype=SEMIDENSE_REPORT_DTYPE)
        check(self._lib.phovo_engine_fetch_semidense_reports(self._h, int(n_pairs), out.ctypes.data),
              "phovo_engine_fetch_semidense_reports")
        return out

    def set_prior_options(self, opt):
        """native.PriorOptions (native.make_prior_options)."""
        check(self._lib.phovo_engine_set_prior_options(self._h, C.byref(opt)), "phovo_engine_set_prior_options")

    def get_prior_options(self):
        opt = native.PriorOptions()
        check(self._lib.phovo_engine_get_prior_options(self._h, C.byref(opt)), "phovo_engine_get_prior_options")
        return opt

    def fetch_prior_reports(self, n_pairs):
        """The records of the last enqueue's pairs, which carried a pose prior, as one structured numpy array of
        PRIOR_REPORT_DTYPE: out["error"][p] = Log(T_p^-1 T), out["prior_cost"][p] = e^T Lambda e."""
        out = np.zeros(int(n_pairs), dtype=PRIOR_REPORT_DTYPE)
        check(self._lib.phovo_engine_fetch_prior_reports(self._h, int(n_pairs), out.ctypes.data),
              "phovo_engine_fetch_prior_reports")
        return out

    def fetch_robust_reports(self, n_pairs):
        """The records of the last enqueue's pairs, which ran under native.OBJECTIVE_INVERSE_ROBUST, as one structured
        numpy array of ROBUST_REPORT_DTYPE: out["delta"][p, L], out["outliers"][p, L]."""
        out = np.zeros(int(n_pairs), dtype=ROBUST_REPORT_DTYPE)
        check(self._lib.phovo_engine_fetch_robust_reports(self._h, int(n_pairs), out.ctypes.data),
              "phovo_engine_fetch_robust_reports")
        return out

    def trust_region_reports(self, n):
        """The solver records of the last enqueue's n pairs (trust-region objective) as one structured numpy array of
        TRUST_REGION_REPORT_DTYPE: out["steps"][p, L], out["termination"][p, L] (native.TR_*), ..."""
        raw = np.zeros(max(n, 1) * native.MAX_LEVELS, dtype=_TR_LEVEL_DTYPE)
        check(self._lib.phovo_engine_fetch_trust_region_reports(self._h, int(n), raw.ctypes.data),
              "phovo_engine_fetch_trust_region_reports")
        raw = raw[:n * native.MAX_LEVELS].reshape(n, native.MAX_LEVELS)
        out = np.zeros(n, dtype=TRUST_REGION_REPORT_DTYPE)
        for name in _TR_LEVEL_DTYPE.names:
            out[name] = raw[name]
        return out

    def get_level_depth_gradients(self, frame, level):
        """Bi-objective: the target's depth-gradient planes (grad_x, grad_y) of one level."""
        w, h = self.level_size(level)
        gx, gy = np.empty((h, w), dtype=np.float64), np.empty((h, w), dtype=np.float64)
        check(self._lib.phovo_engine_get_level_depth_gradients(self._h, int(frame), int(level), gx.ctypes.data,
                                                               gy.ctypes.data), "phovo_engine_get_level_depth_gradients")
        return gx, gy

    def get_level_depth_gain(self, frame, level):
        """Bi-objective: mean(intensity) / mean(depth) of one level of a target frame."""
        g = C.c_double()
        check(self._lib.phovo_engine_get_level_depth_gain(self._h, int(frame), int(level), C.byref(g)),
              "phovo_engine_get_level_depth_gain")
        return g.value

    def set_level_planes(self, frame, level, intensity=None, depth=None, grad_x=None, grad_y=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64)
                for a in (intensity, depth, grad_x, grad_y)]
        w, h = self.level_size(level)
        for a in arrs:
            if a is not None and a.size != w * h:
                raise ValueError("plane size does not match the level")
        ptrs = [a.ctypes.data if a is not None else None for a in arrs]
        check(self._lib.phovo_engine_set_level_planes(self._h, int(frame), int(level), *ptrs),
              "phovo_engine_set_level_planes")

    def get_level_planes(self, frame, level):
        w, h = self.level_size(level)
        outs = [np.empty((h, w), dtype=np.float64) for _ in range(4)]
        check(self._lib.phovo_engine_get_level_planes(self._h, int(frame), int(level),
                                                      *[o.ctypes.data for o in outs]),
              "phovo_engine_get_level_planes")
        return tuple(outs)            # intensity, depth, grad_x, grad_y

    @staticmethod
    def _pairs(src, tgt):
        s = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(tgt, dtype=np.int32).reshape(-1)
        if s.size != t.size:
            raise ValueError("source / target lists differ in length")
        return s, t

    def align_pairs(self, src, tgt, init_states=None, want_reports=False):
        s, t = self._pairs(src, tgt)
        n = s.size
        init = None if init_states is None else np.ascontiguousarray(init_states, dtype=np.float64).reshape(n, 6)
        out = np.zeros((n, 6))
        reps = (native.PairReport * max(n, 1))() if want_reports else None
        ip = C.POINTER(C.c_int)
        check(self._lib.phovo_engine_align_pairs(
            self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
            init.ctypes.data if init is not None else None, out.ctypes.data,
            C.cast(reps, C.c_void_p) if reps is not None else None), "phovo_engine_align_pairs")
        return (out, list(reps)[:n]) if want_reports else out

    def evaluate_pairs(self, src, tgt, states, level, want_structs=False):
        """The Gauss-Newton system of each (source, target) pair at states [n, 6] on `level` (phovo_engine_evaluate_pairs).
        Returns a dict of numpy arrays: information [n, 6, 6], gradient [n, 6], cost [n], rows [n], flags [n]
        (with want_structs, also the native.PairSystem records under "structs")."""
        s, t = self._pairs(src, tgt)
        n = s.size
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(n, 6)
        out = np.zeros(max(n, 1), dtype=PAIR_SYSTEM_DTYPE)         # the C records, written in place
        ip = C.POINTER(C.c_int)
        check(self._lib.phovo_engine_evaluate_pairs(self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip), st.ctypes.data,
                                                    int(level), out.ctypes.data), "phovo_engine_evaluate_pairs")
        out = out[:n]
        res = dict(information=out["information"].reshape(n, 6, 6).copy(), gradient=out["gradient"].copy(),
                   cost=out["cost"].copy(), rows=out["rows"].astype(np.int64), flags=out["flags"].astype(np.int64))
        if want_structs:
            res["structs"] = list((native.PairSystem * n).from_buffer_copy(out.tobytes()))
        return res

    def evaluate_objective_pairs(self, src, tgt, states, level, want_structs=False):
        """The system of each (source, target) pair under the trust-region or the bi-objective objective, whichever the
        engine runs, at states [n, 6] on `level` (phovo_engine_evaluate_objective_pairs).  Returns what evaluate_pairs
        returns: information [n, 6, 6], gradient [n, 6], cost [n] (r^T r: twice the trust region's final_cost), rows [n],
        flags [n] (with want_structs, also the native.PairSystem records under "structs")."""
        s, t = self._pairs(src, tgt)
        n = s.size
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(n, 6)
        out = np.zeros(max(n, 1), dtype=PAIR_SYSTEM_DTYPE)         # the C records, written in place
        ip = C.POINTER(C.c_int)
        check(self._lib.phovo_engine_evaluate_objective_pairs(self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                                              st.ctypes.data, int(level), out.ctypes.data),
              "phovo_engine_evaluate_objective_pairs")
        out = out[:n]
        res = dict(information=out["information"].reshape(n, 6, 6).copy(), gradient=out["gradient"].copy(),
                   cost=out["cost"].copy(), rows=out["rows"].astype(np.int64), flags=out["flags"].astype(np.int64))
        if want_structs:
            res["structs"] = list((native.PairSystem * n).from_buffer_copy(out.tobytes()))
        return res

    def evaluate_inverse_pairs(self, src, tgt, states, level, want_structs=False):
        """The twist-basis system of each (source, target) pair under the inverse-compositional objective at states [n, 6]
        on `level` (phovo_engine_evaluate_inverse_pairs: columns nu, omega of a right-hand twist in the source camera's
        frame).  Returns what evaluate_pairs returns: information [n, 6, 6], gradient [n, 6], cost [n], rows [n], flags [n]
        (with want_structs, also the native.PairSystem records under "structs")."""
        s, t = self._pairs(src, tgt)
        n = s.size
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(n, 6)
        out = np.zeros(max(n, 1), dtype=PAIR_SYSTEM_DTYPE)         # the C records, written in place
        ip = C.POINTER(C.c_int)
        check(self._lib.phovo_engine_evaluate_inverse_pairs(self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                                            st.ctypes.data, int(level), out.ctypes.data),
              "phovo_engine_evaluate_inverse_pairs")
        out = out[:n]
        res = dict(information=out["information"].reshape(n, 6, 6).copy(), gradient=out["gradient"].copy(),
                   cost=out["cost"].copy(), rows=out["rows"].astype(np.int64), flags=out["flags"].astype(np.int64))
        if want_structs:
            res["structs"] = list((native.PairSystem * n).from_buffer_copy(out.tobytes()))
        return res

    def evaluate_robust_pairs(self, src, tgt, states, level, deltas=None, want_structs=False):
        """The weighted twist-basis system of each (source, target) pair under the robust inverse-compositional objective
        at states [n, 6] on `level` (phovo_engine_evaluate_robust_pairs).  deltas None: the threshold is scale_factor times
        the median of |r| at that state; deltas [n], every entry finite and > 0: the caller's own (then median is 0).
        Returns what evaluate_inverse_pairs returns -- information [n, 6, 6], gradient [n, 6], cost [n], rows [n],
        flags [n] -- plus huber_cost, squared_cost, delta, median [n] and outliers [n] (with want_structs, also the
        native.RobustSystem records under "structs")."""
        s, t = self._pairs(src, tgt)
        n = s.size
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(n, 6)
        dl = None
        if deltas is not None:
            dl = np.ascontiguousarray(deltas, dtype=np.float64).reshape(-1)
            if dl.size != n:
                raise ValueError("evaluate_robust_pairs: deltas must have one entry per pair")
            if not (np.all(np.isfinite(dl)) and np.all(dl > 0.0)):
                raise ValueError("evaluate_robust_pairs: every delta must be finite and > 0")
        out = np.zeros(max(n, 1), dtype=ROBUST_SYSTEM_DTYPE)       # the C records, written in place
        ip = C.POINTER(C.c_int)
        check(self._lib.phovo_engine_evaluate_robust_pairs(self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                                           st.ctypes.data, None if dl is None else dl.ctypes.data,
                                                           int(level), out.ctypes.data),
              "phovo_engine_evaluate_robust_pairs")
        out = out[:n]
        res = dict(information=out["information"].reshape(n, 6, 6).copy(), gradient=out["gradient"].copy(),
                   cost=out["cost"].copy(), rows=out["rows"].astype(np.int64), flags=out["flags"].astype(np.int64),
                   huber_cost=out["huber_cost"].copy(), squared_cost=out["squared_cost"].copy(),
                   delta=out["delta"].copy(), median=out["median"].copy(), outliers=out["outliers"].astype(np.int64))
        if want_structs:
            res["structs"] = list((native.RobustSystem * n).from_buffer_copy(out.tobytes()))
        return res

    def evaluate_sampled_pairs(self, src, tgt, states, level, want_structs=False):
        """The Gauss-Newton system of each (source, target) pair under the sampled aligners at states [n, 6] (bilinear
        sampling) or [n, 8] (the affine-illumination objective: pose, alpha, beta) on `level`
        (phovo_engine_evaluate_sampled_pairs).  Returns a dict of numpy arrays: information [n, dim, dim], gradient
        [n, dim], cost [n], rows [n], flags [n] (with want_structs, also the native.SampledSystem records under "structs")."""
        s, t = self._pairs(src, tgt)
        n = s.size
        st = np.ascontiguousarray(states, dtype=np.float64)
        if st.ndim != 2 or st.shape[0] != n or st.shape[1] not in (6, native.SYSTEM_MAX_DIM):
            raise ValueError("states must have shape [n, 6] or [n, 8]")
        dim, ld = st.shape[1], native.SYSTEM_MAX_DIM
        out = np.zeros(max(n, 1), dtype=SAMPLED_SYSTEM_DTYPE)      # the C records, written in place
        ip = C.POINTER(C.c_int)
        check(self._lib.phovo_engine_evaluate_sampled_pairs(self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                                            st.ctypes.data, dim, int(level), out.ctypes.data),
              "phovo_engine_evaluate_sampled_pairs")
        out = out[:n]
        res = dict(information=out["information"].reshape(n, ld, ld)[:, :dim, :dim].copy(),
                   gradient=out["gradient"][:, :dim].copy(), cost=out["cost"].copy(), rows=out["rows"].astype(np.int64),
                   flags=out["flags"].astype(np.int64))
        if want_structs:
            res["structs"] = list((native.SampledSystem * n).from_buffer_copy(out.tobytes()))
        return res

    def evaluate_geometric_pairs(self, src, tgt, states, level):
        """The Gauss-Newton system of each (source, target) pair under the photometric-geometric objective at states [n, 6]
        on `level`, under the engine's geometric options there (phovo_engine_evaluate_geometric_pairs).  Returns a numpy
        record array of GEOMETRIC_SYSTEM_DTYPE, the C records themselves: out["depth_information"][p] is the 36 row-major
        entries of pair p's depth block."""
        s, t = self._pairs(src, tgt)
        n = s.size
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(n, 6)
        out = np.zeros(max(n, 1), dtype=GEOMETRIC_SYSTEM_DTYPE)    # the C records, written in place
        ip = C.POINTER(C.c_int)
        check(self._lib.phovo_engine_evaluate_geometric_pairs(self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
                                                              st.ctypes.data, int(level), out.ctypes.data),
              "phovo_engine_evaluate_geometric_pairs")
        return out[:n].copy()

    def enqueue_align(self, src, tgt, init_states=None, prior_states=None, information=None):
        """phovo_engine_enqueue_align, or, with prior_states [n, 6] and information [n, 6, 6] (both or neither),
        phovo_engine_enqueue_align_prior: a Gaussian pose prior per pair (objectives 5 and 6)."""
        s, t = self._pairs(src, tgt)
        n = s.size
        init = None if init_states is None else np.ascontiguousarray(init_states, dtype=np.float64).reshape(n, 6)
        ip = C.POINTER(C.c_int)
        if (prior_states is None) != (information is None):
            raise ValueError("enqueue_align: prior_states and information go together")
        if prior_states is not None:
            ps = np.ascontiguousarray(prior_states, dtype=np.float64).reshape(n, 6)
            info = np.ascontiguousarray(information, dtype=np.float64).reshape(n, 36)
            check(self._lib.phovo_engine_enqueue_align_prior(
                self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
                init.ctypes.data if init is not None else None, ps.ctypes.data, info.ctypes.data),
                "phovo_engine_enqueue_align_prior")
            return n
        check(self._lib.phovo_engine_enqueue_align(
            self._h, n, s.ctypes.data_as(ip), t.ctypes.data_as(ip),
            init.ctypes.data if init is not None else None), "phovo_engine_enqueue_align")
        return n

    def synchronize(self):
        check(self._lib.phovo_engine_synchronize(self._h), "phovo_engine_synchronize")

    # -- pipelining (phovo_hip.h): PHOVO_ENQUEUE_DEPTH = 2 enqueues in flight, each under a ticket ----------------
    def last_ticket(self):
        return int(self._lib.phovo_engine_last_ticket(self._h))

    def wait(self, ticket):
        check(self._lib.phovo_engine_wait(self._h, int(ticket)), "phovo_engine_wait")

    def fetch(self, ticket, n, want_reports=False):
        out = np.zeros((n, 6))
        reps = (native.PairReport * max(n, 1))() if want_reports else None
        check(self._lib.phovo_engine_fetch(
            self._h, int(ticket), int(n), out.ctypes.data, C.cast(reps, C.c_void_p) if reps is not None else None),
            "phovo_engine_fetch")
        return (out, list(reps)[:n]) if want_reports else out

    def device_states(self, ticket):
        p = C.c_void_p()
        check(self._lib.phovo_engine_device_states(self._h, int(ticket), C.byref(p)), "phovo_engine_device_states")
        return p.value

    def align_ms(self, ticket):
        total = C.c_double()
        per = (C.c_double * native.MAX_LEVELS)()
        check(self._lib.phovo_engine_align_ms(self._h, int(ticket), C.byref(total), per), "phovo_engine_align_ms")
        return total.value, list(per)

    def fetch_results(self, n, want_reports=False):
        out = np.zeros((n, 6))
        reps = (native.PairReport * max(n, 1))() if want_reports else None
        check(self._lib.phovo_engine_fetch_results(
            self._h, int(n), out.ctypes.data, C.cast(reps, C.c_void_p) if reps is not None else None),
            "phovo_engine_fetch_results")
        return (out, list(reps)[:n]) if want_reports else out

    def results_device_ptr(self):
        p = C.c_void_p()
        check(self._lib.phovo_engine_results_device_ptr(self._h, C.byref(p)), "phovo_engine_results_device_ptr")
        return p.value

    def last_align_ms(self):
        total = C.c_double()
        per = (C.c_double * native.MAX_LEVELS)()
        check(self._lib.phovo_engine_last_align_ms(self._h, C.byref(total), per), "phovo_engine_last_align_ms")
        return total.value, list(per)

    def level_launch_info(self, level):
        t, l, o, s = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self._lib.phovo_engine_level_launch_info(self._h, int(level), C.byref(t), C.byref(l),
                                                       C.byref(o), C.byref(s)), "phovo_engine_level_launch_info")
        return dict(threads=t.value, lds_bytes=l.value, owner_in_lds=bool(o.value), source_in_lds=bool(s.value))

    def last_launches(self):
        """The kernel launches of the last enqueue, in order: dicts with levels (coarse to fine), kind, threads,
        lds_bytes, workgroups."""
        if not hasattr(self._lib, "phovo_engine_last_launches"):      # an older build under PHOVO_HIP_LIBRARY (tools/)
            return []
        cap = 4 * native.MAX_LEVELS
        recs = (native.LaunchRecord * cap)()
        n = C.c_int()
        check(self._lib.phovo_engine_last_launches(self._h, C.cast(recs, C.c_void_p), cap, C.byref(n)),
              "phovo_engine_last_launches")
        return [dict(levels=list(range(r.level_first, r.level_last - 1, -1)), kind=native.LAUNCH_KINDS[r.kind],
                     threads=r.threads, lds_bytes=r.lds_bytes, workgroups=r.workgroups) for r in recs[:min(n.value, cap)]]
