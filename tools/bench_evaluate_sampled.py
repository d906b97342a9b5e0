"""Throughput of phovo_engine_evaluate_sampled_pairs (gn_evaluate_sampled_kernels.hip) beside the
scatter phovo_engine_evaluate_pairs of the same build as context: 1024 distinct 640x480 pairs built as bench.py builds them
(consecutive frames of one rendered sequence), each mode evaluated at ITS optimal states from the shipped 4-level file, on
level 0 (640x480) and level 2 (160x120), for 1 pair and for all 1024.  Modes, all on fp64 planes: `bilinear` (corrected
Jacobian), `affine` (8 columns, at the aligner's alpha and beta) and `scatter`.  The three are alternated round by round in
this one process.  Prints one JSON line per case: evaluations/s, ms per call (host wall time of the synchronous C call, the
result copy included) and the share of the 8 TB/s HBM roofline at 40 bytes per pixel (I0, D0, I1, GX1, GY1 once each; the
scatter form's owner-map traffic is left out here so that the three shares have one denominator)."""
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
BYTES_PER_PIXEL = 40.0
W, H = 640, 480
YML = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")
MODES = ("bilinear", "affine", "scatter")


def _engine(mode, seq, n):
    e = odometry.AlignmentEngine(0)
    e.read_configuration_file(YML)
    if mode == "bilinear":
        e.set_extensions(native.make_extensions(sampling=native.SAMPLING_BILINEAR, jacobian_corrected=True))
    elif mode == "affine":
        e.set_objective(native.OBJECTIVE_PHOTOMETRIC_AFFINE)
    e.set_batch_invariant(True)
    e.set_build_all_levels(True)                 # levels 0 and 1 are not optimised by the shipped file, but evaluated here
    e.set_intrinsic_matrix(seq["K"])
    e.reserve_frames(n + 1, W, H)
    e.upload_frames(0, seq["gray"], seq["depth"])
    return e


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
    engines, states = {}, {}
    try:
        for mode in MODES:
            e = engines[mode] = _engine(mode, seq, a.distinct)
            st = e.align_pairs(src, tgt)
            states[mode] = np.hstack([st, e.fetch_illumination(a.distinct)]) if mode == "affine" else st
        for level in [int(v) for v in a.levels.split(",")]:
            lw, lh = engines["scatter"].level_size(level)
            for n in (1, a.distinct):
                calls, outs, times = {}, {}, {m: [] for m in MODES}
                for mode in MODES:
                    e = engines[mode]
                    s_n, t_n, st_n = src[:n].copy(), tgt[:n].copy(), np.ascontiguousarray(states[mode][:n])
                    sampled = mode != "scatter"
                    out = outs[mode] = np.zeros(n, dtype=odometry.SAMPLED_SYSTEM_DTYPE if sampled else odometry.PAIR_SYSTEM_DTYPE)

                    def call(e=e, s_n=s_n, t_n=t_n, st_n=st_n, out=out, sampled=sampled):
                        if sampled:
                            native.check(e._lib.phovo_engine_evaluate_sampled_pairs(
                                e._h, len(s_n), s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip), st_n.ctypes.data,
                                st_n.shape[1], level, out.ctypes.data), "evaluate_sampled")
                        else:
                            native.check(e._lib.phovo_engine_evaluate_pairs(
                                e._h, len(s_n), s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip), st_n.ctypes.data, level,
                                out.ctypes.data), "evaluate")
                    calls[mode] = call
                for _ in range(a.warmup):
                    for mode in MODES:
                        calls[mode]()
                for _ in range(a.steps):                 # alternated: one call of each mode per round
                    for mode in MODES:
                        t0 = time.perf_counter()
                        calls[mode]()
                        times[mode].append(time.perf_counter() - t0)
                for mode in MODES:
                    t = float(np.median(times[mode]))
                    out = outs[mode]
                    print(json.dumps(dict(workload=f"evaluate {lw}x{lh} level {level}", mode=mode, pairs=n,
                                          evaluations_per_s=round(n / t, 1), ms_per_call=round(1e3 * t, 4),
                                          best_ms_per_call=round(1e3 * min(times[mode]), 4), bytes_per_pixel=BYTES_PER_PIXEL,
                                          roofline_share=round(n * lw * lh * BYTES_PER_PIXEL / t / HBM_BYTES_PER_S, 4),
                                          median_rows=int(np.median(out["rows"])),
                                          flagged=int(np.count_nonzero(out["flags"])))), flush=True)
    finally:
        for e in engines.values():
            e.close()


if __name__ == "__main__":
    main()
