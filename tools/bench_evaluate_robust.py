"""Throughput of phovo_engine_evaluate_robust_pairs (gn_evaluate_robust_kernels.hip) beside
phovo_engine_evaluate_inverse_pairs (objective 5, whose kernel this call restates) of the same build: 1024 distinct 640x480
pairs built as bench.py builds them (consecutive frames of one rendered sequence), each call evaluated at ITS aligner's
optimal states from the shipped 4-level file, on level 0 (640x480) and level 2 (160x120), for 1 pair and for all 1024.  ONE
engine and one frame pool serve all three modes: the engine is switched between objective 6 and objective 5 before every call
(outside the timed region), so the calls take turns round by round in this one process on the same frames.
  robust         deltas == NULL: two passes over the pixels (histogram, weighted sums), the median kernel between them
  robust_given   the deltas of a `robust` call handed back: the weighted pass alone
  inverse        objective 5's call: the baseline
Prints one JSON line per case: evaluations/s (median, and the range over the timed runs), ms per call (host wall time of the
synchronous C call, the result copy included) and the share of the 8 TB/s HBM roofline at 40 bytes per pixel per pass over
five planes (I0, D0, GX0, GY0, I1 once each; the histogram pass reads three of them again: 64 bytes per pixel for `robust`)."""
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
BYTES_PER_PIXEL = dict(robust=64.0, robust_given=40.0, inverse=40.0)
W, H = 640, 480
YML = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")
MODES = ("robust", "robust_given", "inverse")
OBJECTIVE = dict(robust=native.OBJECTIVE_INVERSE_ROBUST, robust_given=native.OBJECTIVE_INVERSE_ROBUST,
                 inverse=native.OBJECTIVE_INVERSE_COMPOSITIONAL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--levels", default="0,2")
    a = ap.parse_args()
    seq = synthetic.make_sequence(seed=100, n_frames=a.distinct + 1, width=W, height=H, holes=0.01,
                                  workers=min(16, os.cpu_count() or 1))
    src = np.arange(a.distinct, dtype=np.int32)
    tgt = src + 1
    ip = C.POINTER(C.c_int)
    with odometry.AlignmentEngine(0) as e:
        e.read_configuration_file(YML)
        e.set_batch_invariant(True)
        e.set_build_all_levels(True)                 # levels 0 and 1 are not optimised by the shipped file, but evaluated here
        e.set_intrinsic_matrix(seq["K"])
        e.reserve_frames(a.distinct + 1, W, H)
        e.upload_frames(0, seq["gray"], seq["depth"])
        states = {}
        for mode in ("robust", "inverse"):
            e.set_objective(OBJECTIVE[mode])
            states[mode] = e.align_pairs(src, tgt)
        states["robust_given"] = states["robust"]
        for level in [int(v) for v in a.levels.split(",")]:
            lw, lh = e.level_size(level)
            e.set_objective(OBJECTIVE["robust"])
            own = e.evaluate_robust_pairs(src, tgt, states["robust"], level)["delta"]
            own = np.where(own > 0.0, own, 1.0)                  # (a pair without rows has delta 0, which the call refuses)
            for n in (1, a.distinct):
                calls, outs, times = {}, {}, {m: [] for m in MODES}
                for mode in MODES:
                    s_n, t_n, st_n = src[:n].copy(), tgt[:n].copy(), np.ascontiguousarray(states[mode][:n])
                    d_n = np.ascontiguousarray(own[:n]) if mode == "robust_given" else None
                    inverse = mode == "inverse"
                    out = outs[mode] = np.zeros(n, dtype=odometry.PAIR_SYSTEM_DTYPE if inverse else odometry.ROBUST_SYSTEM_DTYPE)

                    def call(s_n=s_n, t_n=t_n, st_n=st_n, d_n=d_n, out=out, inverse=inverse):
                        if inverse:
                            native.check(e._lib.phovo_engine_evaluate_inverse_pairs(
                                e._h, len(s_n), s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip), st_n.ctypes.data, level,
                                out.ctypes.data), "evaluate_inverse")
                        else:
                            native.check(e._lib.phovo_engine_evaluate_robust_pairs(
                                e._h, len(s_n), s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip), st_n.ctypes.data,
                                None if d_n is None else d_n.ctypes.data, level, out.ctypes.data), "evaluate_robust")
                    calls[mode] = call
                for step in range(a.warmup + a.steps):           # alternated: one call of each mode per round
                    for mode in MODES:
                        e.set_objective(OBJECTIVE[mode])
                        t0 = time.perf_counter()
                        calls[mode]()
                        if step >= a.warmup:
                            times[mode].append(time.perf_counter() - t0)
                for mode in MODES:
                    t = float(np.median(times[mode]))
                    out = outs[mode]
                    line = dict(workload=f"evaluate {lw}x{lh} level {level}", mode=mode, pairs=n, timed_runs=len(times[mode]),
                                evaluations_per_s=round(n / t, 1),
                                evaluations_per_s_range=[round(n / max(times[mode]), 1), round(n / min(times[mode]), 1)],
                                ms_per_call=round(1e3 * t, 4), best_ms_per_call=round(1e3 * min(times[mode]), 4),
                                bytes_per_pixel=BYTES_PER_PIXEL[mode],
                                roofline_share=round(n * lw * lh * BYTES_PER_PIXEL[mode] / t / HBM_BYTES_PER_S, 4),
                                median_rows=int(np.median(out["rows"])), flagged=int(np.count_nonzero(out["flags"])))
                    if mode != "inverse":
                        line["median_outlier_share"] = round(float(np.median(out["outliers"] / np.maximum(out["rows"], 1))), 4)
                    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
