"""Throughput of phovo_engine_evaluate_objective_pairs (the trust-region and the bi-objective system at given states,
gn_evaluate_objective_kernels.hip): 1024 distinct 640x480 pairs built as bench.py builds them (consecutive frames of one
rendered sequence), evaluated at their optimal states under each objective (the shipped 4-level files), on level 0 (640x480)
and level 2 (160x120), for 1 pair and for all 1024.  Prints one JSON line per case: evaluations/s, ms per call (host wall
time of the synchronous C call, the result copy included) and the share of the 8 TB/s HBM roofline at the algorithmic byte
count of DESIGN.md section 18: the fp64 planes read once (trust region: I0, D0, I1, GX1, GY1, 40 bytes per pixel;
bi-objective: those and D1, DGX1, DGY1, 64 bytes) plus 16 bytes of owner-map traffic per pixel.  With --yardstick (default)
phovo_engine_evaluate_pairs runs on the same frames in the same process, at the photometric optima: the figure of section 11
to hold these against."""
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
W, H = 640, 480
YML = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")
YML_CERES = os.path.join(ROOT, "tests", "golden", "ceres", "config_4_level_optimization_ceres.yml")
# name: (objective, plane bytes per pixel, the C call)
OBJECTIVES = {"trust_region": (native.OBJECTIVE_TRUST_REGION, 40.0, "phovo_engine_evaluate_objective_pairs"),
              "biobjective": (native.OBJECTIVE_BIOBJECTIVE, 64.0, "phovo_engine_evaluate_objective_pairs"),
              "photometric": (native.OBJECTIVE_PHOTOMETRIC, 40.0, "phovo_engine_evaluate_pairs")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--levels", default="0,2")
    ap.add_argument("--no-yardstick", dest="yardstick", action="store_false")
    a = ap.parse_args()
    seq = synthetic.make_sequence(seed=100, n_frames=a.distinct + 1, width=W, height=H, holes=0.01,
                                  workers=min(16, os.cpu_count() or 1))
    names = ["trust_region", "biobjective"] + (["photometric"] if a.yardstick else [])
    for name in names:
        objective, plane_bytes, symbol = OBJECTIVES[name]
        with odometry.AlignmentEngine(0) as e:
            if objective == native.OBJECTIVE_TRUST_REGION:
                cfg, opt = native.read_trust_region_file(YML_CERES)
                e.set_config(cfg)
                e.set_objective(objective)
                e.set_trust_region_options(opt)
            else:
                e.set_config(native.read_config_file(YML))
                e.set_objective(objective)
            e.set_batch_invariant(True)
            e.set_build_all_levels(True)             # levels the files do not optimise are evaluated here too
            e.set_intrinsic_matrix(seq["K"])
            e.reserve_frames(a.distinct + 1, W, H)
            e.upload_frames(0, seq["gray"], seq["depth"])
            src = np.arange(a.distinct, dtype=np.int32)
            tgt = src + 1
            states = e.align_pairs(src, tgt)
            fn = getattr(e._lib, symbol)
            for level in [int(v) for v in a.levels.split(",")]:
                lw, lh = e.level_size(level)
                for n in (1, a.distinct):
                    s_n, t_n, st_n = src[:n].copy(), tgt[:n].copy(), np.ascontiguousarray(states[:n])
                    out = np.zeros(n, dtype=odometry.PAIR_SYSTEM_DTYPE)
                    ip = C.POINTER(C.c_int)

                    def call():
                        native.check(fn(e._h, n, s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip), st_n.ctypes.data, level,
                                        out.ctypes.data), symbol)
                    for _ in range(a.warmup):
                        call()
                    times = []
                    for _ in range(a.steps):
                        t0 = time.perf_counter()
                        call()
                        times.append(time.perf_counter() - t0)
                    t = float(np.median(times))
                    per_pixel = plane_bytes + OWNER_BYTES_PER_PIXEL
                    print(json.dumps(dict(workload=f"evaluate {name} {lw}x{lh} level {level}", call=symbol, pairs=n,
                                          evaluations_per_s=round(n / t, 1), ms_per_call=round(1e3 * t, 4),
                                          best_ms_per_call=round(1e3 * min(times), 4), bytes_per_pixel=per_pixel,
                                          roofline_share=round(n * lw * lh * per_pixel / t / HBM_BYTES_PER_S, 4),
                                          median_rows=int(np.median(out["rows"])),
                                          flagged=int(np.count_nonzero(out["flags"])))), flush=True)


if __name__ == "__main__":
    main()
