"""Throughput of phovo_engine_evaluate_geometric_pairs (gn_evaluate_geometric_kernels.hip) beside
phovo_engine_evaluate_sampled_pairs with the corrected bilinear rows on the same frames -- that call is this call's
photometric half, so it is the yardstick: 1024 distinct 640x480 pairs built as bench.py builds them (consecutive frames of
one rendered sequence), evaluated at the photometric-geometric aligner's optimal states from the shipped 4-level file, on
level 0 (640x480) and level 2 (160x120), for 1 pair and for all 1024.  The two calls are alternated round by round in this
one process.  Prints one JSON line per case and mode -- pairs/s, ms per call (host wall time of the synchronous C call, the
result copy included) -- and for the geometric call its rate over the yardstick's and the depth kernel's share of the
8 TB/s HBM roofline at its 16 algorithmic bytes per pixel (D0 and D1 once each), priced at the time the geometric call
takes BEYOND the yardstick's (the two launches that call adds)."""
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
DEPTH_BYTES_PER_PIXEL = 16.0
W, H = 640, 480
YML = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")
MODES = ("geometric", "sampled")


def _engine(mode, seq, n):
    e = odometry.AlignmentEngine(0)
    e.read_configuration_file(YML)
    if mode == "sampled":
        e.set_extensions(native.make_extensions(sampling=native.SAMPLING_BILINEAR, jacobian_corrected=True))
    else:
        e.set_objective(native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
        e.set_geometric_options(native.make_geometric_options(depth_weight=3.0, max_depth_residual=0.1))
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
    engines = {}
    try:
        for mode in MODES:
            engines[mode] = _engine(mode, seq, a.distinct)
        states = engines["geometric"].align_pairs(src, tgt)        # both calls at the geometric aligner's optima
        for level in [int(v) for v in a.levels.split(",")]:
            lw, lh = engines["geometric"].level_size(level)
            for n in (1, a.distinct):
                calls, outs, times = {}, {}, {m: [] for m in MODES}
                for mode in MODES:
                    e = engines[mode]
                    s_n, t_n, st_n = src[:n].copy(), tgt[:n].copy(), np.ascontiguousarray(states[:n])
                    geometric = mode == "geometric"
                    out = outs[mode] = np.zeros(n, dtype=odometry.GEOMETRIC_SYSTEM_DTYPE if geometric
                                                else odometry.SAMPLED_SYSTEM_DTYPE)

                    def call(e=e, s_n=s_n, t_n=t_n, st_n=st_n, out=out, geometric=geometric):
                        if geometric:
                            native.check(e._lib.phovo_engine_evaluate_geometric_pairs(
                                e._h, len(s_n), s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip), st_n.ctypes.data, level,
                                out.ctypes.data), "evaluate_geometric")
                        else:
                            native.check(e._lib.phovo_engine_evaluate_sampled_pairs(
                                e._h, len(s_n), s_n.ctypes.data_as(ip), t_n.ctypes.data_as(ip), st_n.ctypes.data, 6, level,
                                out.ctypes.data), "evaluate_sampled")
                    calls[mode] = call
                for _ in range(a.warmup):
                    for mode in MODES:
                        calls[mode]()
                for _ in range(a.steps):                 # alternated: one call of each mode per round
                    for mode in MODES:
                        t0 = time.perf_counter()
                        calls[mode]()
                        times[mode].append(time.perf_counter() - t0)
                t = {m: float(np.median(times[m])) for m in MODES}
                # the photometric half of the geometric record IS the yardstick's record
                same = bool(np.array_equal(outs["geometric"]["photometric_cost"], outs["sampled"]["cost"]) and
                            np.array_equal(outs["geometric"]["rows"], outs["sampled"]["rows"]))
                for mode in MODES:
                    out = outs[mode]
                    line = dict(workload=f"evaluate {lw}x{lh} level {level}", mode=mode, pairs=n,
                                pairs_per_s=round(n / t[mode], 1), ms_per_call=round(1e3 * t[mode], 4),
                                best_ms_per_call=round(1e3 * min(times[mode]), 4), median_rows=int(np.median(out["rows"])),
                                flagged=int(np.count_nonzero(out["flags"])))
                    if mode == "geometric":
                        extra = t["geometric"] - t["sampled"]
                        line.update(rate_over_sampled=round(t["sampled"] / t["geometric"], 4),
                                    median_depth_rows=int(np.median(out["depth_rows"])),
                                    depth_bytes_per_pixel=DEPTH_BYTES_PER_PIXEL,
                                    depth_roofline_share=(round(n * lw * lh * DEPTH_BYTES_PER_PIXEL / extra / HBM_BYTES_PER_S, 4)
                                                          if extra > 0 else None),
                                    photometric_half_is_the_sampled_record=same)
                    print(json.dumps(line), flush=True)
    finally:
        for e in engines.values():
            e.close()


if __name__ == "__main__":
    main()
