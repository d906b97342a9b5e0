"""Throughput of the trust-region aligner (PHOVO_OBJECTIVE_TRUST_REGION): 640x480, the reference's 4-level Ceres file
(tests/golden/ceres), 8192 pairs drawn from 1024 distinct, built as bench.py builds them: consecutive frames of one
rendered sequence, replicated until the batch is full.  Two modes: the file as shipped, and fixed (every tolerance and
the minimum radius 0: each level runs its 2/4/5/50 steps unless a step is invalid or a test meets an exact zero).
Prints one JSON line per mode: alignments/s, the share of the HBM roofline at 40 algorithmic bytes per
pixel-evaluation (5 fp64 planes: I0, D0, I1, GX1, GY1; taps and owner-map traffic not counted; evaluations counted from
the solver reports), and a parity check of a sample of the timed poses against the CPU checker
(tests/trust_region_ref.py)."""
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
from phovo_amd import native, odometry, synthetic  # noqa: E402
import trust_region_ref as ref  # noqa: E402

HBM_BYTES_PER_S = 8.0e12            # MI355X peak HBM bandwidth
BYTES_PER_PIXEL_EVALUATION = 40
W, H = 640, 480
CFG = os.path.join(ROOT, "tests", "golden", "ceres", "config_4_level_optimization_ceres.yml")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parity-samples", type=int, default=3)
    a = ap.parse_args()
    cfg, shipped = native.read_trust_region_file(CFG)
    nl = cfg.num_levels
    fixed = native.TrustRegionOptions.from_buffer_copy(shipped)
    for L in range(nl):
        fixed.function_tolerance[L] = fixed.gradient_tolerance[L] = fixed.parameter_tolerance[L] = 0.0
        fixed.min_trust_region_radius[L] = 0.0
    ocfg = ref.oracle_config(cfg)
    distinct = max(1, min(a.distinct, a.pairs))
    seq = synthetic.make_sequence(seed=100, n_frames=distinct + 1, width=W, height=H, holes=0.01,
                                  workers=min(16, os.cpu_count() or 1))
    reps = (a.pairs + distinct - 1) // distinct
    src, tgt = [], []
    with odometry.AlignmentEngine(0) as e:
        e.set_config(cfg)
        e.set_intrinsic_matrix(seq["K"])
        e.set_objective(native.OBJECTIVE_TRUST_REGION)
        e.set_batch_invariant(True)
        e.reserve_frames(reps * (distinct + 1), W, H)
        for r in range(reps):                   # every replica has its own copy of the planes in HBM
            base = r * (distinct + 1)
            e.upload_frames(base, seq["gray"], seq["depth"])
            src += [base + t for t in range(distinct)]
            tgt += [base + t + 1 for t in range(distinct)]
        src, tgt = np.array(src[:a.pairs], dtype=np.int32), np.array(tgt[:a.pairs], dtype=np.int32)
        for mode, opt in (("shipped", shipped), ("fixed", fixed)):
            e.set_trust_region_options(opt)
            for _ in range(a.warmup):
                e.align_pairs(src, tgt)
            times = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                out = e.align_pairs(src, tgt)
                times.append(time.perf_counter() - t0)
            rep = e.trust_region_reports(a.pairs)
            launches = e.last_launches()
            evals = 0
            for L in range(nl):
                if cfg.max_num_iterations[L] <= 0:
                    continue
                no_cand = np.isin(rep["termination"][:, L], (native.TR_PARAMETER, native.TR_INVALID_STEP))
                evals += int(np.sum(1 + rep["steps"][:, L] - no_cand)) * (W >> L) * (H >> L)
            rate = a.pairs / float(np.median(times))
            share = evals / a.pairs * rate * BYTES_PER_PIXEL_EVALUATION / HBM_BYTES_PER_S
            worst = 0.0
            for j in range(a.parity_samples):
                t = j * (distinct // max(1, a.parity_samples))          # pair t of the sequence (replica 0)
                xs, _ = ref.align(ocfg, seq["K"], seq["gray"][t], seq["depth"][t], seq["gray"][t + 1], opt)
                d = float(np.abs(out[t] - xs).max())
                worst = max(worst, d) if np.isfinite(d) else float("inf")
            print(json.dumps(dict(workload=f"trust_region 640x480 4-level ceres {mode}", pairs=a.pairs,
                                  distinct_pairs=distinct, alignments_per_s=round(rate, 1),
                                  best_alignments_per_s=round(a.pairs / min(times), 1),
                                  pixel_evaluations_per_pair=round(evals / a.pairs, 1),
                                  roofline_share_40B=round(share, 4), parity_samples=a.parity_samples,
                                  parity_max_state_diff=worst, parity_ok=bool(worst < 1e-9),
                                  mean_steps=[round(float(rep["steps"][:, L].mean()), 2) for L in range(nl)],
                                  launches=[dict(kind=l["kind"], levels=l["levels"], threads=l["threads"],
                                                 lds_bytes=l["lds_bytes"], workgroups=l["workgroups"])
                                            for l in launches])), flush=True)


if __name__ == "__main__":
    main()
