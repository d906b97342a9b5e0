"""Throughput of the photometric-geometric aligner (PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC, sigma = 3, gate 0.1 m) beside the
affine-illumination aligner and the fp64 bilinear-corrected extension, in one process and on the same pairs: 640x480,
config_4_level_optimization_analytic.yml at fixed iterations (thresholds 0: 50 + 20), 8192 pairs drawn from 1024 distinct,
built as bench.py builds them (consecutive frames of one rendered sequence, replicated until the batch is full).  Prints one
JSON line per mode -- alignments/s, the share of the HBM roofline at 48 algorithmic bytes per pixel-iteration (the six fp64
planes I0, D0, I1, GX1, GY1, D1 this objective reads; the other two modes read five and are priced at the same 48 so that the
shares compare as rates do; taps not counted), the level times of the last run (HIP events) -- and a last line with the
ratios.  --mode runs one of the three alone, so that each can sit under a time limit of its own:
    timeout -k 10 300 python tools/bench_geometric.py --mode geometric && timeout -k 10 300 python tools/bench_geometric.py --mode affine"""
import argparse
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
BYTES_PER_PIXEL_ITERATION = 48      # the 6 fp64 planes I0, D0, I1, GX1, GY1, D1, once per iteration
W, H = 640, 480
CFG = os.path.join(ROOT, "config_files", "config_4_level_optimization_analytic.yml")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=["all", "geometric", "affine", "bilinear"], default="all")
    a = ap.parse_args()
    shipped = native.read_config_file(CFG)
    nl = shipped.num_levels
    mi = list(shipped.max_num_iterations[:nl])
    cfg = native.make_config(num_levels=nl, max_iter=mi, min_grad=[0.0] * nl,
                             grad_scale=list(shipped.image_gradients_scaling_factor[:nl]),
                             lam=list(shipped.lambda_optimization_step[:nl]))
    distinct = max(1, min(a.distinct, a.pairs))
    seq = synthetic.make_sequence(seed=100, n_frames=distinct + 1, width=W, height=H, holes=0.01,
                                  workers=min(16, os.cpu_count() or 1))
    reps = (a.pairs + distinct - 1) // distinct
    src, tgt = [], []
    pixel_iterations = sum(mi[L] * (W >> L) * (H >> L) for L in range(nl))
    rates = {}
    with odometry.AlignmentEngine(0) as e:
        e.set_config(cfg)
        e.set_intrinsic_matrix(seq["K"])
        e.reserve_frames(reps * (distinct + 1), W, H)
        for r in range(reps):                   # every replica has its own copy of the planes in HBM
            base = r * (distinct + 1)
            e.upload_frames(base, seq["gray"], seq["depth"])
            src += [base + t for t in range(distinct)]
            tgt += [base + t + 1 for t in range(distinct)]
        src, tgt = np.array(src[:a.pairs], dtype=np.int32), np.array(tgt[:a.pairs], dtype=np.int32)
        e.set_geometric_options(native.make_geometric_options(depth_weight=3.0, max_depth_residual=0.1))
        for mode in ("geometric", "affine", "bilinear"):
            if a.mode not in ("all", mode):
                continue
            if mode == "geometric":             # (fp64 planes in every mode: the pool stays)
                e.set_extensions(native.make_extensions())
                e.set_objective(native.OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
            elif mode == "affine":
                e.set_extensions(native.make_extensions())
                e.set_objective(native.OBJECTIVE_PHOTOMETRIC_AFFINE)
            else:
                e.set_objective(native.OBJECTIVE_PHOTOMETRIC)
                e.set_extensions(native.make_extensions(sampling=native.SAMPLING_BILINEAR, jacobian_corrected=True))
            for _ in range(a.warmup):
                e.align_pairs(src, tgt)
            times, level_ms = [], None
            for _ in range(a.steps):
                t0 = time.perf_counter()
                e.align_pairs(src, tgt)
                times.append(time.perf_counter() - t0)
                level_ms = e.last_align_ms()[1][:nl]
            rates[mode] = a.pairs / float(np.median(times))
            share = pixel_iterations * rates[mode] * BYTES_PER_PIXEL_ITERATION / HBM_BYTES_PER_S
            print(json.dumps(dict(workload=f"{mode} 640x480 4-level analytic fixed", pairs=a.pairs, distinct_pairs=distinct,
                                  alignments_per_s=round(rates[mode], 1),
                                  best_alignments_per_s=round(a.pairs / min(times), 1),
                                  pixel_iterations_per_pair=pixel_iterations, roofline_share_48B=round(share, 4),
                                  level_ms=[round(float(v), 3) for v in level_ms],
                                  launches=[dict(kind=l["kind"], levels=l["levels"], threads=l["threads"],
                                                 workgroups=l["workgroups"]) for l in e.last_launches()])), flush=True)
    if len(rates) == 3:
        print(json.dumps(dict(geometric_over_affine=round(rates["geometric"] / rates["affine"], 4),
                              geometric_over_bilinear=round(rates["geometric"] / rates["bilinear"], 4))), flush=True)


if __name__ == "__main__":
    main()
