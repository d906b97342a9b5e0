"""Throughput of phovo_engine_evaluate_pairs (the Gauss-Newton system at given states, gn_evaluate_kernels.hip): 1024
distinct 640x480 pairs built as bench.py builds them (consecutive frames of one rendered sequence), evaluated at their
optimal states from the shipped 4-level file, on level 0 (640x480) and level 2 (160x120), for 1 pair and for all 1024.
Prints one JSON line per case: evaluations/s, ms per call (host wall time of the synchronous C call, the result copy
included; the Python wrapper's time beside it), and the share of the 8 TB/s HBM roofline at the algorithmic byte count of DESIGN.md section 11: the five planes
in their stored type once (I0, D0, I1, GX1, GY1: 40 / 20 / 12 bytes per pixel for F64 / F32 / F16) plus 16 bytes of owner
map traffic per pixel (pass 1's atomicMax reads and writes 4 bytes, pass 2 reads the entry and puts -1 back)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import phovo_amd  # noqa: E402,F401
from phovo_amd import native, odometry, synthetic  # noqa: E402

HBM_BYTES_PER_S = 8.0e12            # MI355X peak HBM bandwidth
OWNER_BYTES_PER_PIXEL = 16
PLANE_BYTES = {"f64": 40.0, "f32": 20.0, "f16": 12.0}
W, H = 640, 480
YML = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--storage", choices=sorted(PLANE_BYTES), default="f64")
    ap.add_argument("--levels", default="0,2")
    a = ap.parse_args()
    seq = synthetic.make_sequence(seed=100, n_frames=a.distinct + 1, width=W, height=H, holes=0.01,
                                  workers=min(16, os.cpu_count() or 1))
    storage = {"f64": native.STORAGE_F64, "f32": native.STORAGE_F32, "f16": native.STORAGE_F16}[a.storage]
    with odometry.AlignmentEngine(0) as e:
        e.read_configuration_file(YML)
        e.set_extensions(native.make_extensions(plane_storage=storage))
        e.set_batch_invariant(True)
        e.set_build_all_levels(True)             # levels 0 and 1 are not optimised by the shipped file, but evaluated here
        e.set_intrinsic_matrix(seq["K"])
        e.reserve_frames(a.distinct + 1, W, H)
        e.upload_frames(0, seq["gray"], seq["depth"])
        src = np.arange(a.distinct, dtype=np.int32)
        tgt = src + 1
        states = e.align_pairs(src, tgt)
        for level in [int(v) for v in a.levels.split(",")]:
            lw, lh = e.level_size(level)
            for n in (1, a.distinct):
                # the C call alone, into a preallocated record array (what an application pays), then the Python wrapper
                # (which adds the column views) for comparison
                s_n, t_n, st_n = src[:n].copy(), tgt[:n].copy(), np.ascontiguousarray(states[:n])
                out = np.zeros(n, dtype=odometry.PAIR_SYSTEM_DTYPE)
                ip = C.POINTER(C.c_int)

                def call():
                    native.check(e._lib.phovo_engine_evaluate_pairs(e._h, n, s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip),
                                                                    st_n.ctypes.data, level, out.ctypes.data), "evaluate")
                for _ in range(a.warmup):
                    call()
                times = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    call()
                    times.append(time.perf_counter() - t0)
                wrapper = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    r = e.evaluate_pairs(s_n, t_n, st_n, level)
                    wrapper.append(time.perf_counter() - t0)
                assert np.array_equal(r["cost"], out["cost"], equal_nan=True)
                t = float(np.median(times))
                byte_count = n * lw * lh * (PLANE_BYTES[a.storage] + OWNER_BYTES_PER_PIXEL)
                print(json.dumps(dict(workload=f"evaluate {lw}x{lh} level {level}", storage=a.storage, pairs=n,
                                      evaluations_per_s=round(n / t, 1), ms_per_call=round(1e3 * t, 4),
                                      best_ms_per_call=round(1e3 * min(times), 4),
                                      wrapper_ms_per_call=round(1e3 * float(np.median(wrapper)), 4),
                                      bytes_per_pixel=PLANE_BYTES[a.storage] + OWNER_BYTES_PER_PIXEL,
                                      roofline_share=round(byte_count / t / HBM_BYTES_PER_S, 4),
                                      median_rows=int(np.median(out["rows"])), flagged=int(np.count_nonzero(out["flags"])))),
                      flush=True)


if __name__ == "__main__":
    main()
