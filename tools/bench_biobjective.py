"""Throughput of the bi-objective aligner (PHOVO_OBJECTIVE_BIOBJECTIVE): 640x480, the 4-level file in fixed-iteration
mode (20 + 50), 8192 pairs drawn from 1024 distinct, built as bench.py builds them: consecutive frames of one rendered
sequence, replicated until the batch is full.  Prints one JSON line: alignments/s, the share of the HBM roofline at 64
algorithmic bytes per pixel-iteration (8 fp64 planes: I0, D0, I1, D1, GX, GY, DGX, DGY), and a parity check of a sample
of the timed poses against the CPU checker (tests/biobjective_ref.py); a non-finite pose on either side fails it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import phovo_amd  # noqa: E402,F401
from phovo_amd import native, odometry, se3, synthetic  # noqa: E402
from oracle import oracle  # noqa: E402
import biobjective_ref as ref  # noqa: E402

HBM_BYTES_PER_S = 8.0e12            # MI355X peak HBM bandwidth
BYTES_PER_PIXEL_ITERATION = 64
W, H = 640, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parity-samples", type=int, default=3)
    a = ap.parse_args()
    levels, max_iter, min_grad = 4, [0, 0, 20, 50], [0.0] * 4
    kw = dict(num_levels=levels, grad_scale=[0.0625] * 4, lam=[1.0] * 4, max_iter=max_iter, min_grad=min_grad)
    ncfg, ocfg = native.make_config(**kw), oracle.make_config(**kw)
    distinct = max(1, min(a.distinct, a.pairs))
    seq = synthetic.make_sequence(seed=100, n_frames=distinct + 1, width=W, height=H, holes=0.01,
                                  workers=min(16, os.cpu_count() or 1))
    reps = (a.pairs + distinct - 1) // distinct
    src, tgt = [], []
    with odometry.AlignmentEngine(0) as e:
        e.set_config(ncfg)
        e.set_intrinsic_matrix(seq["K"])
        e.set_objective(native.OBJECTIVE_BIOBJECTIVE)
        e.reserve_frames(reps * (distinct + 1), W, H)
        for r in range(reps):                   # every replica has its own copy of the planes in HBM
            base = r * (distinct + 1)
            e.upload_frames(base, seq["gray"], seq["depth"])
            src += [base + t for t in range(distinct)]
            tgt += [base + t + 1 for t in range(distinct)]
        src, tgt = np.array(src[:a.pairs], dtype=np.int32), np.array(tgt[:a.pairs], dtype=np.int32)
        for _ in range(a.warmup):
            e.align_pairs(src, tgt)
        times = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            out = e.align_pairs(src, tgt)
            times.append(time.perf_counter() - t0)
        launches = e.last_launches()
    rate = a.pairs / float(np.median(times))
    pix_it = sum(m * (W >> l) * (H >> l) for l, m in enumerate(max_iter))
    share = rate * pix_it * BYTES_PER_PIXEL_ITERATION / HBM_BYTES_PER_S
    worst = 0.0
    for j in range(a.parity_samples):
        t = j * (distinct // max(1, a.parity_samples))          # pair t of the sequence (replica 0)
        es, *_ = ref.align(ocfg, seq["K"], seq["gray"][t], seq["depth"][t], seq["gray"][t + 1], seq["depth"][t + 1])
        d = se3.state_distance(out[t], es)
        worst = max(worst, d) if np.isfinite(d) else float("inf")
    print(json.dumps(dict(workload="biobjective 640x480 4-level fixed 20+50", pairs=a.pairs, distinct_pairs=distinct,
                          alignments_per_s=round(rate, 1), best_alignments_per_s=round(a.pairs / min(times), 1),
                          roofline_share_64B=round(share, 4), parity_samples=a.parity_samples,
                          parity_max_state_distance=worst, parity_ok=bool(worst < 1e-9),
                          launches=[dict(kind=l["kind"], levels=l["levels"], threads=l["threads"],
                                         lds_bytes=l["lds_bytes"], workgroups=l["workgroups"]) for l in launches])))


if __name__ == "__main__":
    main()
