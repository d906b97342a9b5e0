"""The device-memory ingest without a GPU: the new symbols and their signatures, the descriptor layout as a C compiler
sees it against native.py's ctypes declaration, NULL-engine refusals, the wrapper's TypeErrors, the colour rule in numpy
on its corner cases, and that importing the package does not import torch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(native.library_path())
NEW = ("phovo_engine_upload_frames_device", "phovo_engine_last_ingest", "phovo_odometry_set_source_frame_device",
       "phovo_odometry_set_target_frame_device")


def test_new_symbols_are_exported_with_the_documented_signatures():
    native.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", native.library_path()], capture_output=True, text=True,
                              check=True).stdout
    header = open(os.path.join(ROOT, "include", "phovo_hip.h")).read()
    img, vp = C.POINTER(native.DeviceImage), C.c_void_p
    want = {"phovo_engine_upload_frames_device": [vp, C.c_int, C.c_int, C.c_int, img, img, C.c_double, vp],
            "phovo_engine_last_ingest": [vp, C.POINTER(native.IngestRecord)],
            "phovo_odometry_set_source_frame_device": [vp, img, img, C.c_double, C.c_int, C.c_int, vp],
            "phovo_odometry_set_target_frame_device": [vp, img, img, C.c_double, C.c_int, C.c_int, vp]}
    for name in NEW:
        assert re.search(rf"\bT {name}\b", exported), name
        res, args = native.SYMBOLS[name]
        assert res is C.c_int and args == want[name], name
        # the header declares as many parameters as native.py binds
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(args), (name, decl)


def test_descriptor_layout_matches_native_py_and_null_engines_are_refused(tmp_path):
    native.lib()
    exe = tmp_path / "device_image_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "device_image_layout.c"), "-o", str(exe),
                           "-L", PKG, "-lphovo_hip", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for line, struct in ((lines[0], native.DeviceImage), (lines[1], native.IngestRecord)):
        tok = line.split()
        assert int(tok[2]) == C.sizeof(struct)
        seen = dict(zip(tok[3::2], (int(v) for v in tok[4::2])))
        assert seen == {name: getattr(struct, name).offset for name, _ in struct._fields_}
    assert [int(v) for v in lines[2].split()[1:]] == [native.IMAGE_U8_GRAY, native.IMAGE_U8_RGB, native.IMAGE_U8_BGR,
                                                      native.IMAGE_F64, native.IMAGE_F32, native.IMAGE_F16, native.IMAGE_U16]
    assert lines[3] == "null refusals ok"


def test_null_engine_refusals_through_ctypes():
    L = native.lib()
    img = native.DeviceImage(0, 0, 0, native.IMAGE_U8_GRAY, 0)
    assert L.phovo_engine_upload_frames_device(None, 0, 1, 3, C.byref(img), None, 1.0, None) == native.E_INVALID_ARGUMENT
    assert "null engine" in L.phovo_last_error().decode()
    assert L.phovo_odometry_set_source_frame_device(None, C.byref(img), C.byref(img), 1.0, 4, 4, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_odometry_set_source_frame_device(None, C.byref(img), None, 1.0, 4, 4, None) == native.E_INVALID_ARGUMENT
    assert "depth" in L.phovo_last_error().decode()
    assert L.phovo_odometry_set_target_frame_device(None, C.byref(img), None, 1.0, 4, 4, None) == native.E_INVALID_ARGUMENT
    assert L.phovo_engine_last_ingest(None, None) == native.E_INVALID_ARGUMENT


def test_the_wrapper_refuses_host_memory_and_unsupported_dtypes():
    import torch
    g = torch.zeros((2, 4, 6), dtype=torch.uint8)
    with pytest.raises(TypeError, match="host memory"):
        odometry._device_images(g, None, "rgb", None, 0, batched=True)
    with pytest.raises(TypeError, match="host memory"):
        odometry._device_images(np.zeros((2, 4, 6), np.uint8), None, "rgb", None, 0, batched=True)
    with pytest.raises(TypeError):
        odometry._device_images([[1, 2], [3, 4]], None, "rgb", None, 0, batched=False)
    # dtypes are looked at before the device is
    with pytest.raises(TypeError, match="uint8"):
        odometry._device_images(torch.zeros((2, 4, 6), dtype=torch.float32), None, "rgb", None, 0, batched=True)
    for bad in (torch.bfloat16, torch.int32, torch.uint8):
        with pytest.raises(TypeError, match="float64"):
            odometry._device_tensor(torch.zeros((2, 4, 6), dtype=bad), "depth", tuple(odometry._depth_formats()))
    assert odometry._depth_formats()[torch.int16] == native.IMAGE_U16


def test_the_colour_rule_in_numpy_on_the_corner_colours():
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8)
    got = odometry.gray_from_colour(corners)
    # (9797 R + 19234 G + 3737 B + 16384) >> 15 by hand: the weights sum to 32768, so white stays 255 and black 0
    want = [0, (3737 * 255 + 16384) >> 15, (19234 * 255 + 16384) >> 15, ((19234 + 3737) * 255 + 16384) >> 15,
            (9797 * 255 + 16384) >> 15, ((9797 + 3737) * 255 + 16384) >> 15, ((9797 + 19234) * 255 + 16384) >> 15, 255]
    assert got.tolist() == want == [0, 29, 150, 179, 76, 105, 226, 255]
    assert 9797 + 19234 + 3737 == 1 << 15
    np.testing.assert_array_equal(odometry.gray_from_colour(corners[:, ::-1], "bgr"), got)
    gray = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(odometry.gray_from_colour(np.stack([gray] * 3, axis=-1)), gray)      # gray stays gray
    with pytest.raises(ValueError):
        odometry.gray_from_colour(corners.astype(np.int32))
    with pytest.raises(ValueError):
        odometry.gray_from_colour(corners, "grb")


def test_importing_the_package_does_not_import_torch():
    code = ("import sys; import phovo_amd; from phovo_amd import native, odometry, sequence; "
            "assert 'torch' not in sys.modules, 'torch was imported'; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
