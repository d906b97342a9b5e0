// Internal declarations shared by the host engine and the HIP kernels (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "phovo_hip.h"

namespace phovo_hip {

// Planes of one frame at one level, in pool order.
enum Plane { PLANE_I = 0, PLANE_D = 1, PLANE_GX = 2, PLANE_GY = 3, PLANES_PER_FRAME = 4 };

// Everything one Gauss-Newton level launch needs (passed by value as the kernel argument,
// so the scalars land in SGPRs).
struct GNLevelArgs {
  int w, h, n;              // level size, n = w*h
  int level;
  int max_iter;             // max_num_iterations[level] (> 0)
  int n_chunks;             // ceil(n / 64)
  double lambda;            // lambda_optimization_step[level]
  double min_grad_norm;     // min_gradient_norm[level]
  double fx, fy, ox, oy, ifx, ify;   // level-scaled intrinsics (...Analytic.h:203-209)
  double min_depth, max_depth;
  double huber_delta;       // > 0: Huber IRLS weights (extension, not in the reference); <= 0: off
  const unsigned char *planes;   // pool of this level: frame f at planes + f*frame_bytes,
  size_t frame_bytes;            //   plane p of a frame at + plane_off[p], n elements of the storage type
  size_t plane_off[PLANES_PER_FRAME];
  const int *src;           // [pairs] source frame of each pair
  const int *tgt;           // [pairs] target frame of each pair
  double *states;           // [pairs][6] in: initial / previous level, out: updated
  phovo_pair_report *reports;   // [pairs]
  int *g_owner;             // [pairs][n] owner map in global memory (only when it does not fit LDS)
  unsigned long long *g_mask;   // [pairs][n_chunks] in-bounds ballots in global memory (only when they do not fit LDS either:
                                // levels above ~1.27 M pixels), else null
  int n_pairs;              // pairs of this launch
  int *work_counter;        // [QUEUES_PER_LEVEL] heads QUEUE_HEAD_STRIDE ints apart, zeroed before the launch: workgroups draw pair indices from them
  int n_queues;             // 1: one queue for the whole grid; 8: one per XCD over a contiguous eighth of the pairs (+ stealing)
  int n_lds;                // owner map in HBM only: its first n_lds entries (a multiple of 64) live in LDS instead
  int slide_m;              // sliding-window kernel: bands a target may lie away from its source's band (gn_slide_reach_bands)
  int depth_lds_chunks;     // owner map in LDS: the depth of the first this-many 64-pixel chunks is kept in leftover LDS by pass 1
                            // and read from there by pass 2 (0: none)
  // Hand-over of pairs from the sliding-window launch of a level to the exact launch right behind it (same stream).  A
  // list is [n_pairs + 1] ints, zeroed before the first launch: pair indices, and at [n_pairs] their number.
  //   handover_out  non-null (sliding-window kernel): a pair whose warp leaves the window is appended there (its state and
  //                 its completed iteration count, reports[p].iterations[level], are in place)
  //   handover_in   non-null: the launch works on that list instead of the pairs 0..n_pairs-1 and continues every pair at
  //                 its stored iteration count; takeover_flag is OR-ed into reports[p].flags of every pair taken
  const int *handover_in;
  int *handover_out;
  unsigned takeover_flag;
  size_t rec_off;           // bilinear sampling: byte offset, in a frame, of its TAP RECORDS {I, GX, GY, pad} (pyr_build_tap_records)
};

// Several consecutive levels of one launch (gn_fused_kernel): lv[0] is the coarsest.  The pair list, states, reports and
// the queue are those of lv[0]; every level shares them.
constexpr int GN_MAX_FUSED_LEVELS = 3;
struct GNFusedArgs {
  GNLevelArgs lv[GN_MAX_FUSED_LEVELS];
  int n_levels;
  int n_max;                // pixels of the largest level: sizes the owner map in LDS
  int n_pairs;
  int n_queues;
  int *work_counter;
};

constexpr int QUEUES_PER_LEVEL = 8;      // one per XCD
constexpr int QUEUE_HEAD_STRIDE = 32;    // ints between two queue heads: a 128-byte line each (the draws are atomics, served per line)
constexpr int QUEUE_HEADS_INTS = QUEUES_PER_LEVEL * QUEUE_HEAD_STRIDE;     // the heads of one launch

struct GNLaunchPlan {
  int variant;              // which instantiation of the level kernel (gn_kernels.hip)
  int threads;              // workgroup size
  int wgs_per_cu;           // workgroups of this geometry that fit one CU (sizes the persistent grid)
  int lds_bytes;            // dynamic LDS
  bool owner_in_lds;
  bool source_in_lds;
  int owner_lds_entries;    // owner map in HBM: how many of its leading entries the leftover LDS holds (GNLevelArgs::n_lds)
  bool mask_in_hbm;         // owner map in HBM and a level so large that the per-chunk ballots do not fit LDS either
  int depth_lds_chunks;     // leading 64-pixel chunks whose depth pass 1 parks in the LDS this geometry leaves unused (GNLevelArgs)
};

// Chooses the launch geometry for a level of n pixels.  Returns false if the level cannot be
// handled (inbound-mask does not fit LDS).
// prefer_latency 1: the geometry for a handful of pairs (each alone on a CU): 512 threads instead of four workgroups of 256.
// bound_by_bytes: the planes are fp64 (the level kernels are then bound by bytes at the fabric and a geometry may be chosen
// for the depth it can park in LDS; with narrow storages they are bound by the vector unit)
bool gn_plan_level(int n, GNLaunchPlan *plan, int prefer_latency = 0, bool bound_by_bytes = true);
// args.n_pairs pairs, args.work_counter zeroed on the stream beforehand; the grid is min(pairs, CUs x workgroups/CU).
hipError_t gn_launch_level(const GNLevelArgs &args, const GNLaunchPlan &plan, int storage, int cu_count,
                           hipStream_t stream);
// Several consecutive levels in ONE persistent launch (a pair flows through them inside the workgroup that drew it): every
// level must be gn_level_fusable (owner map in LDS beside a second 512-thread workgroup on the CU).
bool gn_level_fusable(int n_pixels);
int gn_fused_lds_bytes(int n_max);
bool gn_plan_fused_geometry(int n_pixels, GNLaunchPlan *plan);      // the per-level kernel in the fused launch's geometry
hipError_t gn_launch_fused(const GNFusedArgs &args, int storage, int cu_count, hipStream_t stream);
// Extension (PHOVO_SAMPLING_BILINEAR): single-pass kernels, 256 threads, no owner map, any level size (fp64 / fp32 planes:
// taps through LDS-DMA; fp16 planes: tap records).
hipError_t gn_launch_level_bilinear(const GNLevelArgs &args, int storage, bool corrected, int cu_count,
                                    hipStream_t stream);
int gn_bilinear_wgs_per_cu(int storage);      // workgroups of the bilinear kernel for that plane storage that stay resident per CU
// Wide form (gn_wide_kernels.hip): many workgroups per pair, three launches per iteration; for a handful of
// pairs on large levels.  fp64 planes, reference semantics only.
size_t gn_wide_workspace_bytes(int n, int n_pairs);
hipError_t gn_run_level_wide(const GNLevelArgs &args, int n_pairs, void *workspace, int *h_done_scratch,
                             hipStream_t stream);
hipError_t gn_prepare_kernels();   // raises the dynamic-LDS limit of every instantiation
// Evaluation of the Gauss-Newton system at given states (gn_evaluate_kernels.hip, phovo_engine_evaluate_pairs): one level,
// nearest / scatter sampling, any plane storage, optional Huber weights.
struct GNEvalArgs {
  int w, h, n, n_chunks;
  double fx, fy, ox, oy, ifx, ify;   // level-scaled intrinsics, as GNLevelArgs
  double min_depth, max_depth;
  double huber_delta;                // > 0: Huber IRLS weights at the given state
  const unsigned char *planes;       // pool of the level (GNLevelArgs)
  size_t frame_bytes;
  size_t plane_off[PLANES_PER_FRAME];
  const int *src, *tgt;              // [pairs of the group]
  const double *states;              // [pairs of the group][6]
};
int gn_eval_tiles(int n);                          // 1024-pixel tiles of a level of n pixels
size_t gn_eval_slab_doubles_per_pair(int n);       // doubles of tile sums per pair
// g_owner: [n_pairs][n] int32 holding -1 everywhere (and again on return); g_mask: [n_pairs][n_chunks];
// g_part: [n_pairs][gn_eval_slab_doubles_per_pair(n)]; out: [n_pairs] on the device.
hipError_t gn_eval_pairs(const GNEvalArgs &a, int n_pairs, int storage, int *g_owner, unsigned long long *g_mask,
                         double *g_part, phovo_pair_system *out, hipStream_t stream);
// The same for the rows the sampled aligners define (gn_evaluate_sampled_kernels.hip, phovo_engine_evaluate_sampled_pairs):
// bilinear sampling with either Jacobian (state_dim 6, any plane storage, optional Huber weights) and the
// affine-illumination rows (state_dim 8: pose, alpha, beta; fp64 planes, no Huber weights).  No owner map, no ballots.
struct GNSampledEvalArgs {
  int w, h, n, n_chunks;
  int state_dim;                     // 6 or 8
  double fx, fy, ox, oy, ifx, ify;   // level-scaled intrinsics, as GNLevelArgs
  double min_depth, max_depth;
  double huber_delta;                // > 0: Huber IRLS weights at the given state (state_dim 6 only)
  const unsigned char *planes;       // pool of the level (GNLevelArgs)
  size_t frame_bytes;
  size_t plane_off[PLANES_PER_FRAME];
  const int *src, *tgt;              // [pairs of the group]
  const double *states;              // [pairs of the group][state_dim]
};
size_t gn_eval_sampled_slab_doubles_per_pair(int n, int dim);      // doubles of tile sums per pair (dim 6 or 8)
// g_part: [n_pairs][gn_eval_sampled_slab_doubles_per_pair(n, state_dim)]; out: [n_pairs] on the device.
hipError_t gn_eval_sampled_pairs(const GNSampledEvalArgs &a, int n_pairs, int storage, bool corrected, double *g_part,
                                 phovo_sampled_system *out, hipStream_t stream);
// Bi-objective (intensity + depth) form (gn_biobjective_kernel.hip, PHOVO_OBJECTIVE_BIOBJECTIVE): fp64 planes, nearest /
// scatter sampling.  Every frame of the level carries, beside the four planes, the target's depth gradients (fp64 planes at
// dgx_off / dgy_off) and its depth gain mean(I) / mean(D) (one double at gain_off).
struct GNBiObjectiveArgs {
  GNLevelArgs lv;
  size_t dgx_off, dgy_off, gain_off;
};
// Geometry for a level of n pixels: owner map in LDS where it fits (256 threads, two per CU; else 512 threads, one per
// CU), else in HBM (lv.g_owner: [pairs][n]).  False: the level is too large (more than 2 097 151 pixels).
bool gn_plan_level_biobjective(int n, GNLaunchPlan *plan);
hipError_t gn_prepare_biobjective_kernels();
hipError_t gn_launch_level_biobjective(const GNBiObjectiveArgs &args, const GNLaunchPlan &plan, int cu_count,
                                       hipStream_t stream);
// Trust-region (Levenberg-Marquardt) form (gn_trust_region_kernel.hip, PHOVO_OBJECTIVE_TRUST_REGION): fp64 planes, the
// photometric objective's frames; bilinear samples of the target, the owner-map row rule, the LM loop inside the workgroup.
struct GNTrustRegionArgs {
  GNLevelArgs lv;                    // (lambda, min_grad_norm and huber_delta unused; max_iter = max_num_iterations[level])
  int max_iterations;
  double function_tolerance, gradient_tolerance, parameter_tolerance;
  double initial_radius, max_radius, min_radius, min_relative_decrease;
  phovo_trust_region_report *tr_reports;   // [pairs], zeroed before the first level
};
// Geometry for a level of n pixels: owner map in LDS where it fits (256 threads, two per CU; else 512 threads, one per
// CU), else in HBM (lv.g_owner: [workgroups][n], the grid being min(pairs, CUs x wgs_per_cu)).  False: the level is too
// large (more than 2 097 151 pixels).
bool gn_plan_level_trust_region(int n, GNLaunchPlan *plan);
hipError_t gn_prepare_trust_region_kernels();
hipError_t gn_launch_level_trust_region(const GNTrustRegionArgs &args, const GNLaunchPlan &plan, int cu_count,
                                        hipStream_t stream);
// Evaluation of the trust-region and the bi-objective system at given states (gn_evaluate_objective_kernels.hip,
// phovo_engine_evaluate_objective_pairs): fp64 planes, the tile form of gn_eval_pairs, gn_eval_tiles(n) tiles per pair.
struct GNObjectiveEvalArgs {
  int w, h, n, n_chunks;
  double fx, fy, ox, oy, ifx, ify;   // level-scaled intrinsics, as GNLevelArgs
  double min_depth, max_depth;       // the depth range in force at the call
  const unsigned char *planes;       // pool of the level (GNLevelArgs)
  size_t frame_bytes;
  size_t plane_off[PLANES_PER_FRAME];
  size_t dgx_off, dgy_off, gain_off; // bi-objective: the target's depth gradients and gain (GNBiObjectiveArgs)
  const int *src, *tgt;              // [pairs of the group]
  const double *states;              // [pairs of the group][6]
};
// objective: PHOVO_OBJECTIVE_TRUST_REGION or PHOVO_OBJECTIVE_BIOBJECTIVE.  g_owner: [n_pairs][n] int32 holding -1
// everywhere (and again when the launches have run); g_mask: [n_pairs][n_chunks]; g_part: [n_pairs]
// [gn_eval_slab_doubles_per_pair(n)]; out: [n_pairs] on the device.
hipError_t gn_eval_objective_pairs(const GNObjectiveEvalArgs &a, int objective, int n_pairs, int *g_owner,
                                   unsigned long long *g_mask, double *g_part, phovo_pair_system *out, hipStream_t stream);
// Affine-illumination form (gn_affine_kernel.hip, PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE): fp64 planes, the photometric
// objective's frames; the bilinear extension's rows with the true warp Jacobian, the residual I1 - (1 + alpha) I0 - beta and
// an 8 x 8 system per iteration.  No owner map, any level size, 256 threads.
struct GNAffineArgs {
  GNLevelArgs lv;                    // (huber_delta and rec_off unused)
  double *illum;                     // [pairs][2] alpha, beta: in: previous level (zeros at the first), out: updated
};
int gn_affine_wgs_per_cu();          // workgroups of the kernel that stay resident per CU
int gn_affine_lds_bytes();
hipError_t gn_launch_level_affine(const GNAffineArgs &args, int cu_count, hipStream_t stream);
// Photometric-geometric form (gn_geometric_kernel.hip, PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC): fp64 planes, the photometric
// objective's frames; the affine form's rows at alpha = beta = 0 and, per row, a depth row on the target's depth plane (the
// one a source upload of the target frame left in the pool).  No owner map, any level size, 256 threads.
struct GNGeometricArgs {
  GNLevelArgs lv;                    // (huber_delta and rec_off unused)
  double depth_weight;               // sigma_L (> 0)
  double max_depth_residual;         // the residual gate of the level; <= 0: off
  phovo_geometric_report *geo_reports;   // [pairs], zeroed before the first level
};
int gn_geometric_wgs_per_cu();       // workgroups of the kernel that stay resident per CU
int gn_geometric_lds_bytes();
hipError_t gn_launch_level_geometric(const GNGeometricArgs &args, int cu_count, hipStream_t stream);
// Evaluation of that objective's system at given states (gn_evaluate_geometric_kernels.hip,
// phovo_engine_evaluate_geometric_pairs): the photometric block through gn_eval_sampled_pairs (corrected rows, fp64 planes,
// no Huber weights), the depth block through a tile kernel of the same form, both into one phovo_geometric_system.
struct GNGeometricEvalArgs {
  GNSampledEvalArgs s;               // state_dim 6, huber_delta 0
  double depth_weight;               // sigma_L (> 0)
  double max_depth_residual;         // the residual gate of the level; <= 0: off
};
// g_part_sampled, g_part_depth: [n_pairs][gn_eval_sampled_slab_doubles_per_pair(n, 6)] each; sampled, out: [n_pairs] on
// the device.
hipError_t gn_eval_geometric_pairs(const GNGeometricEvalArgs &args, int n_pairs, double *g_part_sampled,
                                   phovo_sampled_system *sampled, double *g_part_depth, phovo_geometric_system *out,
                                   hipStream_t stream);
// Inverse-compositional form (gn_inverse_kernel.hip, PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL): fp64 planes, the photometric
// objective's frames; the bilinear extension's rows and residual, the Jacobian from the SOURCE frame's gradient planes (the
// ones a target upload of the source frame left in the pool), the step composed on SE(3).  No owner map, any level size,
// 256 threads.
struct GNInverseArgs {
  GNLevelArgs lv;                    // (huber_delta and rec_off unused)
};
int gn_inverse_wgs_per_cu();         // workgroups of the kernel that stay resident per CU
int gn_inverse_lds_bytes();
hipError_t gn_launch_level_inverse(const GNInverseArgs &args, int cu_count, hipStream_t stream);
// Robust inverse-compositional form (gn_inverse_robust_kernel.hip, PHOVO_OBJECTIVE_INVERSE_ROBUST): the same rows, residual,
// Jacobian and step, every row under a Huber weight whose threshold is scale_factor times the median of |r| over the pair's
// rows, taken from a 4096-bin histogram in LDS and lagging one iteration.  256 threads.
struct GNInverseRobustArgs {
  GNLevelArgs lv;                    // (huber_delta and rec_off unused)
  double scale_factor;               // phovo_robust_options: finite, > 0
  phovo_robust_report *rob_reports;  // [pairs], zeroed before the first level
};
int gn_inverse_robust_wgs_per_cu();
int gn_inverse_robust_lds_bytes();
hipError_t gn_launch_level_inverse_robust(const GNInverseRobustArgs &args, int cu_count, hipStream_t stream);
// Semi-dense inverse-compositional form (gn_inverse_semidense_kernel.hip, PHOVO_OBJECTIVE_INVERSE_SEMIDENSE):
// objective 5's rows on the source pixels selected once per pair and level by depth and gradient magnitude.  256 threads.
// records: [grid][slab_records] 4-byte records, grid = min(pairs, CUs x gn_inverse_semidense_wgs_per_cu()); a workgroup
// touches the slab at blockIdx.x alone.  seg_records = gn_inverse_semidense_segment_records(lv.n_chunks) is one wave's
// segment of THIS level; slab_records >= gn_inverse_semidense_slab_records(lv.n_chunks) (the enqueue's largest level's).
struct GNInverseSemiDenseArgs {
  GNLevelArgs lv;                    // (huber_delta and rec_off unused)
  double tau2;                       // min_pixel_gradient[level] squared in fp64
  unsigned *records;
  size_t slab_records;
  int seg_records;
  phovo_semidense_report *sd_reports;   // [pairs], zeroed before the first level
};
int gn_inverse_semidense_wgs_per_cu();
int gn_inverse_semidense_lds_bytes();
int gn_inverse_semidense_segment_records(int n_chunks);
size_t gn_inverse_semidense_slab_records(int n_chunks);
hipError_t gn_launch_level_inverse_semidense(const GNInverseSemiDenseArgs &args, int cu_count, hipStream_t stream);
// The two forms above (5 and 6) under a Gaussian pose prior (gn_inverse_prior_kernel.hip, phovo_engine_enqueue_align_prior, DESIGN.md
// §24): one template over `robust`.  prior: [pairs][GN_PRIOR_DOUBLES] -- R_p row-major (9), t_p (3), the upper triangle of
// Lambda row-major (21), and 1.0 where Lambda has a non-zero entry, else 0.0.
constexpr int GN_PRIOR_DOUBLES = 34;
struct GNInversePriorArgs {
  GNLevelArgs lv;                    // (huber_delta and rec_off unused)
  double scale_factor;               // robust only, as GNInverseRobustArgs
  phovo_robust_report *rob_reports;  // robust only
  const double *prior;               // [pairs][GN_PRIOR_DOUBLES]
  phovo_prior_report *prior_reports; // [pairs], zeroed before the first level
  double level_scale;                // phovo_prior_options.level_scale[level]: finite, >= 0
};
int gn_inverse_prior_wgs_per_cu();
int gn_inverse_prior_lds_bytes(bool robust);
hipError_t gn_launch_level_inverse_prior(const GNInversePriorArgs &args, bool robust, int cu_count, hipStream_t stream);
// Evaluation of that objective's system at given states, in the twist basis (gn_evaluate_inverse_kernels.hip,
// phovo_engine_evaluate_inverse_pairs): fp64 planes, the tile form of gn_eval_sampled_pairs, gn_eval_tiles(n) tiles per
// pair, no owner map, no ballots.  The source frame's gradient planes are read (a target upload's).
struct GNInverseEvalArgs {
  int w, h, n, n_chunks;
  double fx, fy, ox, oy, ifx, ify;   // level-scaled intrinsics, as GNLevelArgs
  double min_depth, max_depth;       // the depth range in force at the call
  const unsigned char *planes;       // pool of the level (GNLevelArgs)
  size_t frame_bytes;
  size_t plane_off[PLANES_PER_FRAME];
  const int *src, *tgt;              // [pairs of the group]
  const double *states;              // [pairs of the group][6]
};
// g_part: [n_pairs][gn_eval_slab_doubles_per_pair(n)]; out: [n_pairs] on the device.
hipError_t gn_eval_inverse_pairs(const GNInverseEvalArgs &a, int n_pairs, double *g_part, phovo_pair_system *out,
                                 hipStream_t stream);
// The weighted system of the robust inverse-compositional objective at given states (gn_evaluate_robust_kernels.hip,
// phovo_engine_evaluate_robust_pairs): the same args and tile form.  g_hist: [n_pairs][4096] words, cleared here on the
// stream in front of the histogram launch; g_md: [n_pairs][2] doubles (m, delta) -- written by the median kernel, or, with
// deltas_given, filled by the caller with (0, delta) before the call, and then neither g_hist nor scale_factor is used.
hipError_t gn_eval_robust_pairs(const GNInverseEvalArgs &a, int n_pairs, double scale_factor, bool deltas_given,
                                unsigned *g_hist, double *g_md, double *g_part, phovo_robust_system *out, hipStream_t stream);
// Sliding-window form for levels whose owner map exceeds LDS (gn_slide_kernel.hip): owner ring in LDS; pairs whose
// motion leaves the window are appended to args.handover_out for a follow-up gn_launch_level that takes that list.
hipError_t gn_prepare_slide_kernels();
hipError_t gn_launch_level_slide(const GNLevelArgs &args, int storage, int cu_count, hipStream_t stream);
size_t gn_slide_lds_bytes();
int gn_slide_threads();
int gn_slide_reach_bands(int w, int h);      // GNLevelArgs::slide_m for a level of w x h pixels

// Pyramid producers (SetSourceFrame / SetTargetFrame, ...Analytic.h:466-491), batched over `frames`
// consecutive frames: frame f reads src + f*src_frame_stride and writes dst + f*dst_frame_stride (elements).
hipError_t pyr_intensity_level(const uint8_t *gray, size_t src_frame_stride, int frames, int w, int h, int level,
                               int lw, int lh, double *dst, size_t dst_frame_stride, hipStream_t stream);
hipError_t pyr_depth_level(const double *depth, size_t src_frame_stride, int frames, int w, int h, int level,
                           int lw, int lh, double *dst, size_t dst_frame_stride, hipStream_t stream);
hipError_t pyr_depth_level_u16(const uint16_t *depth, size_t src_frame_stride, double scale, int frames, int w,
                               int h, int level, int lw, int lh, double *dst, size_t dst_frame_stride,
                               hipStream_t stream);
hipError_t pyr_scharr(const double *base, size_t frame_stride, size_t img_off, size_t gx_off, size_t gy_off,
                      int frames, int w, int h, double scale, hipStream_t stream);
// fp64 <-> storage-type plane conversion (storage = PHOVO_STORAGE_*, is_depth selects the depth element type).
size_t storage_elem_size(int storage, bool is_depth);
hipError_t pyr_store_plane(const double *src, size_t src_frame_stride, int frames, int n, unsigned char *dst,
                           size_t dst_frame_bytes, int storage, bool is_depth, hipStream_t stream);
hipError_t pyr_load_plane(const unsigned char *src, int n, double *dst, int storage, bool is_depth,
                          hipStream_t stream);
// Bilinear sampling (extension): one interleaved record {I, GX, GY, pad} per pixel of a target frame, in the planes' own
// storage type (the same bits as the three planes), so that a bilinear tap is one or two wide loads instead of three
// gathers: frames consecutive frames of a level pool, planes at plane_off[] and the records at rec_off in every frame.
hipError_t pyr_build_tap_records(unsigned char *pool, size_t frame_bytes, const size_t plane_off[PLANES_PER_FRAME],
                                 size_t rec_off, int frames, int n, int storage, hipStream_t stream);
// Bi-objective target planes (BuildDepthDerivativesPyramids, ...BiObjective.h:214-240): Scharr of depth * (1.0/max_depth),
// where inv_max_depth is that quotient, with the frame layout of pyr_scharr.
hipError_t pyr_scharr_scaled(const double *base, size_t frame_stride, size_t img_off, size_t gx_off, size_t gy_off,
                             int frames, int w, int h, double inv_max_depth, double scale, hipStream_t stream);
// Per frame: mean(intensity) / mean(depth) over all n pixels (:300), each mean summed in a fixed order, written to
// base + f*frame_stride + gain_off (elements).
hipError_t pyr_depth_gain(const double *base, size_t frame_stride, size_t img_off, size_t depth_off, size_t gain_off,
                          int frames, int n, hipStream_t stream);
hipError_t pyr_gaussian_blur(double *img, double *tmp, int w, int h, int ksize,
                             const double *d_kernel, hipStream_t stream);
hipError_t fill_i32(int *dst, size_t n, int value, hipStream_t stream);

// ingest_kernels.hip: packs `frames` strided frames of a PHOVO_IMAGE_* format from device memory into packed staging
// (u8 gray -> u8, u16 -> u16, f64 / f32 / f16 -> f64 with the scale applied to f32 and f16).  *wide tells which form ran.
int ingest_source_pixel_bytes(int format);     // 0: unknown format
hipError_t ingest_pack(int format, const void *src, size_t row_stride, size_t frame_stride, int frames, int w, int h,
                       double scale, void *dst, bool *wide, hipStream_t stream);

// Diagnostic switches read from the environment exist only in a -DPHOVO_TUNING build (tools/); the release library reads
// PHOVO_VISUALIZE_DIR and nothing else.
#ifdef PHOVO_TUNING
bool tuning_switch(const char *name);
#else
inline bool tuning_switch(const char *) { return false; }
#endif

// Error plumbing
void set_last_error(const std::string &msg);
int fail(int status, const std::string &msg);

// OpenCV-FileStorage-dialect reader (yml_config.cpp)
int read_config_file(const char *path, phovo_config *cfg);
int read_extensions_file(const char *path, phovo_extensions *ext);
int read_trust_region_file(const char *path, phovo_config *cfg, phovo_trust_region_options *opt);
int read_geometric_file(const char *path, phovo_geometric_options *opt);
int read_semidense_file(const char *path, phovo_semidense_options *opt);

}  // namespace phovo_hip
