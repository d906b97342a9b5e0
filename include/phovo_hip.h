/*
 * phovo_hip.h -- C ABI of the MI355X-native analytic Gauss-Newton RGB-D alignment path.
 *
 * This is the drop-in boundary for ONE path of MiguelAlgaba/photoconsistency-visual-odometry:
 *   phovo::Analytic::CPhotoconsistencyOdometryAnalytic<unsigned char,double>
 *   (phovo/include/CPhotoconsistencyOdometryAnalytic.h:57-608), i.e. the abstract surface of
 *   phovo/include/CPhotoconsistencyOdometry.h:137-179 plus SetMinDepth/SetMaxDepth/
 *   ReadConfigurationFile.
 * The reference has no FFI: its "plugin API" is that C++ template class.  The functions
 * below are what a binding of that class binds (include/phovo/CPhotoconsistencyOdometryAnalytic.h
 * in this repository is such a binding; INTEGRATION.md shows it next to the reference's apps).
 * Plain pointers and sizes only; every function returns a phovo_status (0 = ok) and never throws.
 * All images are row-major; strides are in BYTES; the library copies what it is given (the
 * caller keeps ownership of every buffer, as with the reference's const& arguments,
 * ...Analytic.h:466-491).  All arithmetic is fp64 on the device.
 *
 * Two layers:
 *   phovo_odometry_*  one frame pair at a time -- 1:1 with the reference's methods.
 *   phovo_engine_*    the batched form the throughput path uses: a pool of frames whose
 *                     pyramids live in HBM and a list of (source, target) frame pairs that
 *                     are aligned by one launch per active pyramid level.
 * A process drives one engine per GPU; engines are independent (one HIP stream each).
 */
#ifndef PHOVO_HIP_H
#define PHOVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHOVO_MAX_LEVELS 16

typedef enum phovo_status {
  PHOVO_OK = 0,
  PHOVO_E_INVALID_ARGUMENT = 1,  /* NULL pointer, index out of range                         */
  PHOVO_E_CONFIG = 2,            /* missing / malformed key, per-level array too short        */
  PHOVO_E_SHAPE = 3,             /* frame size does not match the pool, level too large       */
  PHOVO_E_HIP = 4,               /* a HIP runtime call failed (message: phovo_last_error())   */
  PHOVO_E_NOT_READY = 5,         /* call order violated (e.g. Optimize before Set*Frame)      */
  PHOVO_E_IO = 6,                /* file cannot be opened                                     */
  PHOVO_E_UNSUPPORTED = 7        /* a mode the device path does not implement                 */
} phovo_status;

/* Flags in phovo_pair_report.flags */
#define PHOVO_PAIR_NONFINITE 1u  /* J^T J was singular / the state became inf or NaN: the reference
                                    propagates inf/NaN silently (...Analytic.h:540); so does this
                                    library, but it says so here.                                 */
#define PHOVO_PAIR_WINDOW_FALLBACK 2u  /* informational: on a level whose owner map exceeds LDS this pair's warp left
                                    the sliding window of the fast kernel (a displacement of more than about 20 rows of
                                    the level, e.g. a large in-plane rotation) and the exact kernel with the map in HBM
                                    finished it.  In linear index a uniform displacement D stays inside iff
                                    -(m - 1) * 1536 <= D <= m * 1536, m the level's reach in bands: forward 15 360 pixels
                                    at 640x480 (m = 10) and 9 216 at 320x240 (m = 6), backward 13 824 and 7 680.  The
                                    result is the same; only the time differs.                                   */
#define PHOVO_PAIR_RANK_DEFICIENT 4u  /* fewer than six Jacobian rows were filled in SOME iteration of some level (the
                                    flag is sticky; phovo_pair_report.valid_pixels holds the count of each level's last
                                    iteration): J^T J was singular by construction there and the step taken from it
                                    rounding noise -- finite or not -- exactly as in the reference, which inverts such a
                                    matrix without a word (...Analytic.h:540).                                        */

/* The per-level parameter vectors of the reference (...Analytic.h:91-103), as filled by
 * ReadConfigurationFile (:581-607) or by the constructor defaults (:430-443). */
typedef struct phovo_config {
  int    num_levels;                                       /* numOptimizationLevels                      */
  int    blur_filter_size[PHOVO_MAX_LEVELS];               /* blurFilterSize (at each level)             */
  double image_gradients_scaling_factor[PHOVO_MAX_LEVELS]; /* imageGradientsScalingFactor (at each level)*/
  double lambda_optimization_step[PHOVO_MAX_LEVELS];       /* lambda_optimization_step (at each level)   */
  int    max_num_iterations[PHOVO_MAX_LEVELS];             /* max_num_iterations (at each level)         */
  double min_gradient_norm[PHOVO_MAX_LEVELS];              /* min_gradient_norm (at each level)          */
  int    visualize_iterations;                             /* visualizeIterations: the reference shows |I1 - warped|
                                                              in a window after every iteration (:551-557); here
                                                              phovo_odometry_optimize writes that image to
                                                              $PHOVO_VISUALIZE_DIR/optimize_imgDiff_level<L>_iteration<N>.pgm
                                                              when the variable is set, and ignores the key otherwise */
} phovo_config;

/* What Optimize() did for one pair (the reference only prints this behind
 * ENABLE_PRINT_CONSOLE_OPTIMIZATION_PROGRESS, ...Analytic.h:396-422). */
typedef struct phovo_pair_report {
  int      iterations[PHOVO_MAX_LEVELS]; /* m_Iteration when each level stopped (:547-549)      */
  double   gradient_norm;                /* ||J^T r|| of the last executed iteration (:380)      */
  uint32_t flags;                        /* PHOVO_PAIR_*                                         */
  uint32_t reserved;
  int32_t  valid_pixels[PHOVO_MAX_LEVELS]; /* rows of J filled in the LAST executed iteration of each level: source
                                            pixels that passed the depth gate (:280) and whose warp landed inside the
                                            image (:302-303); 0 for a level with max_num_iterations == 0.  A handful of
                                            them (a rank-deficient J^T J) is what precedes PHOVO_PAIR_NONFINITE.   */
} phovo_pair_report;

/* The Gauss-Newton system of one frame pair at a given state on one level (phovo_engine_evaluate_pairs,
 * phovo_odometry_get_pair_system) -- not in the reference, which forms it in every iteration and discards it.
 * Its rows are exactly those ComputeResidualsAndJacobians (...Analytic.h:191-367) fills at that state on that level:
 * the depth gate (:280) and the round() bounds test (:297-303), the residual scattered to the rounded target index
 * with the last source pixel in raster order winning (:358), the target gradients read at the SOURCE index
 * (:346-347), and the reference's Jacobian INCLUDING its transcription slip `temp11 = cos(pitch)*cos(yaw) + x` (:253):
 * this is the matrix the aligner inverts (:538-540), not the normal matrix of the true warp Jacobian.  With
 * huber_delta[level] > 0 the rows carry the aligner's IRLS weights at that state (w = 1 if |r| <= delta, delta/|r|
 * otherwise); else W = I.  The parameterisation is the state's: (x, y, z, yaw, pitch, roll).  A caller that turns
 * `information` into a covariance (its inverse, scaled by cost / (rows - 6) for example) gets the covariance of that
 * parameterisation under that Jacobian.
 * Relation to the aligner: the system the aligner solves in iteration k of a level is this system at the state the
 * iteration starts from; after its last system the aligner always takes one more step, so the system AT the returned
 * state is a pass of its own.  Arithmetic: fp64 on the device; the sums are taken in an order that depends on the
 * level size only, so a pair's result is the same bit for bit whatever the batch, its position in it, or the engine's
 * fusion, latency-form and batch-invariant settings. */
typedef struct phovo_pair_system {
  double   information[36]; /* J^T W J, row-major, exactly symmetric (filled from the upper triangle)            */
  double   gradient[6];     /* J^T W r                                                                          */
  double   cost;            /* r^T W r over the reference's residual vector, which is indexed by TARGET pixel:
                               every target pixel with an owner counts, filled Jacobian row or not             */
  int32_t  rows;            /* rows of J filled: the count phovo_pair_report.valid_pixels uses                  */
  uint32_t flags;           /* PHOVO_PAIR_RANK_DEFICIENT if rows < 6, PHOVO_PAIR_NONFINITE if any sum is inf/NaN */
} phovo_pair_system;

/* The Gauss-Newton system of one frame pair under the SAMPLED aligners at a given state on one level
 * (phovo_engine_evaluate_sampled_pairs, phovo_odometry_get_sampled_system): the bilinear extension
 * (PHOVO_SAMPLING_BILINEAR, dim 6) and the affine-illumination objective (PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE, dim 8:
 * pose, alpha, beta).  Its rows are the ones those aligners fill at that state: every source pixel in raster order that
 * passes the strict depth gate min_depth < D0 < max_depth and whose nearest target pixel is inside the image
 * (-0.5 < u < W - 0.5, -0.5 < v < H - 0.5); I1, GX1 and GY1 sampled bilinearly from four taps with every index clamped to
 * the image; residual and Jacobian row both belong to the source pixel.  Columns: with jacobian_corrected = 0 the
 * reference's Jacobian including its temp11 slip (:253), with 1 the true warp Jacobian; under the affine objective the
 * true one plus dr/dalpha = -I0 and dr/dbeta = -1, with r = I1(u, v) - (1 + alpha) I0 - beta.  With huber_delta[level] > 0
 * (dim 6 only) the rows carry the aligner's IRLS weights at that state (w = 1 if |r| <= delta, delta/|r| otherwise) in
 * information, gradient and cost.  The 8 x 8 system also yields the pose covariance with gain and offset marginalised
 * out (a Schur complement on the caller's side).
 * Relation to the aligner: the system it solves in iteration k of a level is this system at the state the iteration starts
 * from (on fp64 planes up to one rounding of the sample in the outer half-pixel band, gn_bilinear_kernel.hip).
 * Arithmetic: fp64 on the device; the sums are taken in an order that depends on the level size only, so a pair's result
 * is the same bit for bit whatever the batch, its position in it, or the engine's settings. */
#define PHOVO_SYSTEM_MAX_DIM 8
typedef struct phovo_sampled_system {
  double   information[64]; /* J^T W J, row-major with leading dimension 8, exactly symmetric (filled from the upper
                               triangle); rows and columns >= dim are 0 */
  double   gradient[8];     /* J^T W r; entries >= dim are 0 */
  double   cost;            /* r^T W r over the rows */
  int32_t  rows;            /* rows of J filled: the count phovo_pair_report.valid_pixels uses */
  uint32_t flags;           /* PHOVO_PAIR_RANK_DEFICIENT if rows < dim, PHOVO_PAIR_NONFINITE if any sum is inf/NaN */
  int32_t  dim;             /* 6 or 8 */
  int32_t  reserved;
} phovo_sampled_system;

/* ---- extensions that are NOT in the reference (BASELINE.json configs[4]); all off by default -------------
 * plane_storage: how the pyramid planes are kept in HBM.  Arithmetic is fp64 in every mode; pyramids are built
 * in fp64 and rounded once when stored (fp64 -> fp32 by round-to-nearest-even, fp16 via fp32).
 *   PHOVO_STORAGE_F64  reference-exact (cv::Mat_<double>, ...Analytic.h:73-85)
 *   PHOVO_STORAGE_F32  all four planes fp32  (half the HBM footprint and traffic)
 *   PHOVO_STORAGE_F16  intensity and gradients fp16, depth fp32  (10 instead of 32 bytes per pixel)
 * huber_delta[L] > 0 turns the least-squares step of level L into an IRLS step of the Huber loss: residual k gets
 * the weight 1 if |r_k| <= delta, delta/|r_k| otherwise, in both J^T W J and J^T W r (and hence in the gradient norm
 * of the termination test).  <= 0: off. */
#define PHOVO_STORAGE_F64 0
#define PHOVO_STORAGE_F32 1
#define PHOVO_STORAGE_F16 2
/* sampling: how the target frame is looked up.
 *   PHOVO_SAMPLING_NEAREST_SCATTER  the reference's analytic path: C round() of the warped position, residual
 *                                   scattered to the target index, Jacobian row at the source index (...Analytic.h:297-358)
 *   PHOVO_SAMPLING_BILINEAR         forward-additive alignment with bilinear samples of intensity and gradients at the
 *                                   real-valued warped position (in bounds iff the nearest pixel is, taps clamped to
 *                                   the edge); residual and Jacobian row both belong to the source pixel: no scatter.
 * jacobian_corrected (bilinear sampling only): 1 = the true warp Jacobian, i.e. without the reference's
 * `temp11 = cos(pitch)*cos(yaw)+x` transcription slip (...Analytic.h:253); 0 = the reference's Jacobian. */
#define PHOVO_SAMPLING_NEAREST_SCATTER 0
#define PHOVO_SAMPLING_BILINEAR 1
typedef struct phovo_extensions {
  int    plane_storage;                     /* PHOVO_STORAGE_*            yml: "plane_storage_bits: 64|32|16" */
  int    sampling;                          /* PHOVO_SAMPLING_*           yml: "sampling_bilinear: 0|1"       */
  int    jacobian_corrected;                /* 0 | 1                      yml: "jacobian_corrected: 0|1"      */
  int    reserved;
  double huber_delta[PHOVO_MAX_LEVELS];     /* optional yml key "huber_delta (at each level)"             */
} phovo_extensions;

/* Objective (phovo_engine_set_objective):
 *   PHOVO_OBJECTIVE_PHOTOMETRIC  the reference's method 0, CPhotoconsistencyOdometryAnalytic (default)
 *   PHOVO_OBJECTIVE_BIOBJECTIVE  the reference's method 2, CPhotoconsistencyOdometryBiObjective: photometric and depth
 *                                error together over 2N rows, reproduced with the reference's row collisions (last
 *                                writer wins).  Target frames keep their depth: their uploads need it and
 *                                build the target depth pyramid, the depth-gradient planes (Scharr of
 *                                depth * (1.0/max_depth), with the max depth in force at upload) and the per-level gain
 *                                mean(intensity) / mean(depth).  Reference-exact only: fp64 planes, nearest / scatter
 *                                sampling, no Huber weights -- anything else is PHOVO_E_UNSUPPORTED, from
 *                                phovo_engine_set_objective or phovo_engine_set_extensions, whichever comes second.
 *                                Fusion, sliding-window, wide and latency-form settings are accepted and have no
 *                                effect.  phovo_pair_report: valid_pixels counts contributing source pixels,
 *                                PHOVO_PAIR_RANK_DEFICIENT means fewer than 6 of them. */
#define PHOVO_OBJECTIVE_PHOTOMETRIC 0
#define PHOVO_OBJECTIVE_BIOBJECTIVE 1
/*   PHOVO_OBJECTIVE_TRUST_REGION the reference's method 1, CPhotoconsistencyOdometryCeres: the photometric residual with
 *                                bilinear samples of the target at the real-valued warped position, the exact warp
 *                                Jacobian (no temp11 slip) and a Levenberg-Marquardt trust-region solver per level with
 *                                function, gradient and parameter tolerances (phovo_trust_region_options; DESIGN.md §12
 *                                has the contract, a reading of Ceres 1.14's TrustRegionMinimizer).  Frames are the
 *                                photometric objective's: switching between the two keeps the frame pool.
 *                                Reference-exact only: fp64 planes, nearest / scatter sampling setting, no Huber
 *                                weights, jacobian_corrected 0 -- anything else is PHOVO_E_UNSUPPORTED, whichever setter
 *                                comes second; phovo_engine_evaluate_pairs is PHOVO_E_UNSUPPORTED too (this objective's
 *                                system is phovo_engine_evaluate_objective_pairs).  Fusion,
 *                                sliding-window, wide and latency-form settings are accepted and have no effect.
 *                                phovo_pair_report: iterations[L] = LM steps (iteration 0 not counted), valid_pixels[L] =
 *                                owned targets at the final point, gradient_norm = ||J^T r||_2 there (of the last level
 *                                run), PHOVO_PAIR_NONFINITE when an evaluation was not finite or the state is not (a
 *                                NaN / inf initial state: no pixel warps, the level ends without a step and the state
 *                                stays as given), PHOVO_PAIR_RANK_DEFICIENT when fewer than 6 rows remain.  The
 *                                per-level solver record is phovo_trust_region_report. */
#define PHOVO_OBJECTIVE_TRUST_REGION 2
/*   PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE  not in the reference: the photometric residual with a per-pair gain and offset,
 *                                r_k = I1(u_k, v_k) - (1 + alpha) I0_k - beta, estimated jointly with the pose (8 entries per
 *                                pair: x, y, z, yaw, pitch, roll, alpha, beta; DESIGN.md §14 has the contract).  The rows are
 *                                those of the bilinear extension with jacobian_corrected = 1 -- source pixels in raster
 *                                order, bilinear samples of I1, GX1, GY1 at the real-valued warped position (clamped taps; in
 *                                bounds iff the nearest pixel is), the true warp Jacobian -- with two columns appended,
 *                                dr/dalpha = -I0_k and dr/dbeta = -1.  The level loop is that extension's with 8 in place
 *                                of 6 (H = J^T J is 8 x 8; min_gradient_norm is tested on ||J^T r||_2 over all 8 entries);
 *                                every pair starts at alpha = beta = 0 and both carry from level to level with the pose.
 *                                Frames are the photometric objective's: switching between objectives 0, 2 and 3 keeps the
 *                                frame pool.  Supported: fp64 planes, the default sampling setting, no Huber weights,
 *                                jacobian_corrected 0 -- anything else is PHOVO_E_UNSUPPORTED, whichever setter comes
 *                                second; phovo_engine_evaluate_pairs is PHOVO_E_UNSUPPORTED too.  Fusion, sliding-window,
 *                                wide, latency-form and batch-invariant settings are accepted and have no effect.
 *                                out_states and phovo_engine_device_states stay n x 6 (the pose); alpha and beta are read
 *                                with phovo_engine_fetch_illumination.  phovo_pair_report keeps its meaning: valid_pixels[L]
 *                                = rows of the level's last iteration, PHOVO_PAIR_RANK_DEFICIENT when fewer than 8 rows
 *                                were filled in some iteration, PHOVO_PAIR_NONFINITE as under the photometric objective. */
#define PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE 3
/*   PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC  not in the reference: intensity and depth together on the bilinear rows (6 entries
 *                                per pair, the pose; DESIGN.md §16 has the contract).  The photometric rows are those of the
 *                                affine-illumination objective at alpha = beta = 0: r_I = I1(u, v) - I0 on every source pixel
 *                                that passes the depth gate and whose nearest target pixel is inside the image, bilinear
 *                                samples on clamped taps, the true warp Jacobian.  Such a pixel adds a depth row
 *                                r_D = sigma_L (D1(u, v) - Z') iff the four taps of the TARGET's depth all pass
 *                                min_depth < d < max_depth (NaN fails) and, with max_depth_residual[L] > 0,
 *                                |D1(u, v) - Z'| <= max_depth_residual[L]; Z' is the third coordinate of the moved point,
 *                                D1(u, v) the bilinear sample with the intensity's taps and weights, and
 *                                J_D = sigma_L (dgx dU/dp + dgy dV/dp - dZ'/dp) with (dgx, dgy) the exact derivative of
 *                                that interpolant (at an integer u or v the cell towards +u / +v: floor).  H = sum J_I
 *                                J_I^T + sum J_D J_D^T, g likewise; the level loop is the
 *                                bilinear extension's.  sigma_L and the residual limit are phovo_geometric_options.
 *                                The target's depth on level L is the depth plane a SOURCE upload of that frame leaves
 *                                there (what phovo_engine_get_level_planes returns as depth): target frames need
 *                                PHOVO_ROLE_BOTH, and an enqueue whose target lacks the source role on an active level is
 *                                PHOVO_E_NOT_READY.  No new planes: switching between objectives 0, 2, 3 and 4 keeps the
 *                                frame pool.  Supported: fp64 planes, the default sampling setting, no Huber weights,
 *                                jacobian_corrected 0 -- anything else is PHOVO_E_UNSUPPORTED, whichever setter comes
 *                                second; both evaluate calls are PHOVO_E_UNSUPPORTED too: this objective's system, with
 *                                the photometric and the depth block kept apart, is phovo_geometric_system
 *                                (phovo_engine_evaluate_geometric_pairs, phovo_odometry_get_geometric_system).  Fusion,
 *                                sliding-window, wide, latency-form and batch-invariant settings are accepted and have no
 *                                effect.
 *                                phovo_pair_report: valid_pixels[L] = photometric rows of the level's last iteration,
 *                                PHOVO_PAIR_RANK_DEFICIENT when fewer than 6 photometric rows were filled in some iteration,
 *                                PHOVO_PAIR_NONFINITE as under the photometric objective, gradient_norm = ||g||_2 of the
 *                                last system.  Depth rows and the two costs: phovo_geometric_report. */
#define PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC 4
/*   PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL  not in the reference: the photometric residual aligned inverse-compositionally
 *                                (Baker & Matthews; 6 entries per pair, the pose; DESIGN.md §20 has the contract).  Per
 *                                level L and pair, with the level's scaled intrinsics (line numbers: ...Analytic.h):
 *                                  entry   (R, t) = eigenPose(state).
 *                                  rows    the bilinear extension's: every source pixel k in raster order with
 *                                          min_depth < D0_k < max_depth (NaN fails); p = (px, py, pz) as at :282-283,
 *                                          P' = R p + t, (u, v) as at :295-296; in bounds iff -0.5 < u < W - 0.5 and
 *                                          -0.5 < v < H - 0.5; I1(u, v) bilinear on four clamped taps;
 *                                          r_k = I1(u, v) - I0_k.
 *                                  J_k     from the SOURCE alone, twist order (nu_x, nu_y, nu_z, omega_x, omega_y, omega_z):
 *                                          g = (GX0_k, GY0_k) from the source frame's gradient planes as stored (the
 *                                          gradient scaling factor included),
 *                                          a = (g_x fx / pz, g_y fy / pz, -(a_0 px + a_1 py) / pz),  J_k = (a, p x a).
 *                                  step    H = sum J J^T, g = sum J r, xi = -lambda_L H^-1 g,
 *                                          (R, t) <- (R E_R, R E_t + t) with (E_R, E_t) = Exp(xi) on SE(3) (Rodrigues,
 *                                          E_t = V nu; for |omega|^2 < 1e-8 the coefficients' Taylor series through
 *                                          |omega|^4).  R is not re-orthonormalised.
 *                                  end     after the step when iteration + 1 >= max_num_iterations[L], else when
 *                                          ||g||_2 < min_gradient_norm[L] (g in the TWIST basis: the shipped thresholds
 *                                          were tuned on Euler-basis gradients, the two coincide near zero rotation only),
 *                                          and, with PHOVO_PAIR_NONFINITE, when an entry of (R, t) is not finite.
 *                                  exit    state = (t, yaw = atan2(R10, R00), pitch = atan2(-R20, sqrt(R00^2 + R10^2)),
 *                                          roll = atan2(R21, R22)); a non-finite (R, t) gives a NaN state.  Levels are
 *                                          separate launches, the n x 6 state array is all that travels between them;
 *                                          levels with max_num_iterations 0 are not launched.
 *                                The source's gradient planes on level L are those a TARGET upload of that frame leaves
 *                                there: source frames need PHOVO_ROLE_BOTH, and an enqueue whose source lacks the target
 *                                role on an active level is PHOVO_E_NOT_READY.  No new planes: switching between objectives
 *                                0, 2, 3, 4 and 5 keeps the frame pool.  Supported: fp64 planes, the default sampling
 *                                setting, no Huber weights, jacobian_corrected 0 -- anything else is PHOVO_E_UNSUPPORTED,
 *                                whichever setter comes second.  Its system, in the twist basis, is
 *                                phovo_engine_evaluate_inverse_pairs / phovo_odometry_get_inverse_system; the four other
 *                                phovo_engine_evaluate_* calls and phovo_odometry_get_*_system calls, which speak the
 *                                Euler basis, stay PHOVO_E_UNSUPPORTED under this objective.  Fusion, sliding-window, wide, latency-form and
 *                                batch-invariant settings are accepted and have no effect.
 *                                phovo_pair_report keeps its meaning: iterations[L], valid_pixels[L] = rows of the level's
 *                                last system, gradient_norm = ||g||_2 of the last system, PHOVO_PAIR_RANK_DEFICIENT
 *                                (sticky) when a system had fewer than 6 rows. */
#define PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL 5
/*   PHOVO_OBJECTIVE_INVERSE_ROBUST  not in the reference: the inverse-compositional aligner under a Huber weight whose
 *                                threshold follows the pair's own residuals (DESIGN.md §22 has the contract).  Per level L
 *                                and pair:
 *                                  rows    entry, rows, r_k and J_k exactly as under PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL.
 *                                  hist    4096 bins of width 2^-12 over |r| of the rows: with q = fabs(r) * 4096.0 the bin
 *                                          is q < 4096.0 ? (int)q : 4095 (|r| >= 1 and a NaN residual: the last bin).
 *                                  median  n rows, half = (n + 1) / 2 in integers, k the first bin whose cumulative count
 *                                          reaches half, before the count below bin k, h[k] the count in it:
 *                                          m = ((double)k + (double)(half - before) / (double)h[k]) * 0x1p-12 in fp64, in
 *                                          that order; n = 0 gives m = 0.  delta = scale_factor * m (phovo_robust_options).
 *                                  lag     delta_0 from a histogram-only pass at the level's entry pose; iteration i builds
 *                                          its system with delta_i, and delta_{i+1} is the median rule on iteration i's
 *                                          residuals (so delta_1 = delta_0).
 *                                  system  w = fabs(r) <= delta_i ? 1.0 : delta_i / fabs(r); H = sum w J J^T, g = sum w J r;
 *                                          outliers = rows with fabs(r) > delta_i.
 *                                  step    xi = -lambda_L H^-1 g, composition, termination (||g||_2 of the WEIGHTED g), the
 *                                          finite test, the flags and the level's exit as under objective 5.
 *                                phovo_robust_report has the delta and the outliers of every level's last system.  Source
 *                                frames need PHOVO_ROLE_BOTH (else PHOVO_E_NOT_READY), as under objective 5; switching between
 *                                objectives 0, 2, 3, 4, 5 and 6 keeps the frame pool.  Supported: fp64 planes, the default
 *                                sampling setting, no huber_delta extension, jacobian_corrected 0 -- anything else is
 *                                PHOVO_E_UNSUPPORTED, whichever setter comes second.  Its weighted system, in the twist basis, is
 *                                phovo_engine_evaluate_robust_pairs / phovo_odometry_get_robust_system; the five other
 *                                phovo_engine_evaluate_* calls and their phovo_odometry_get_*_system calls stay
 *                                PHOVO_E_UNSUPPORTED under this objective.  phovo_pair_report keeps its meaning. */
#define PHOVO_OBJECTIVE_INVERSE_ROBUST 6
/*   PHOVO_OBJECTIVE_INVERSE_SEMIDENSE  not in the reference: the inverse-compositional aligner on the source pixels worth a
 *                                row (DESIGN.md §25 has the contract).  Per level L and pair:
 *                                  select  once, before the first iteration: source pixel k is SELECTED iff
 *                                          min_depth < D0_k < max_depth and GX0_k*GX0_k + GY0_k*GY0_k >= tau_L*tau_L, in fp64
 *                                          on the gradient planes as stored (the gradient scaling factor included; the
 *                                          sum may or may not be contracted); NaN fails either comparison.  tau_L =
 *                                          phovo_semidense_options.min_pixel_gradient[L].  The selection depends on the
 *                                          source frame, the level and tau_L only.
 *                                  rows    the selected pixels whose warp lands in bounds; for a selected pixel the warp, the
 *                                          bounds test, the taps, r_k and J_k are objective 5's.
 *                                  step    step, end and exit exactly as under PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL.
 *                                So this is objective 5 on a source whose depth is NaN wherever the pixel is not selected;
 *                                the order of summation is the kernel's own, results agree with that within rounding, and a
 *                                pair's bits depend on nothing but the pair.  phovo_semidense_report has the number of
 *                                selected pixels per level; phovo_pair_report keeps its meaning (valid_pixels[L] = rows of
 *                                the level's last system).  Source frames need PHOVO_ROLE_BOTH (else PHOVO_E_NOT_READY);
 *                                switching between objectives 0, 2, 3, 4, 5, 6 and 7 keeps the frame pool.  Supported: fp64
 *                                planes, the default sampling setting, no Huber weights, jacobian_corrected 0 -- anything
 *                                else is PHOVO_E_UNSUPPORTED, whichever setter comes second.  A level wider or taller than
 *                                65535 pixels is PHOVO_E_SHAPE at the enqueue (a list record is col | row << 16).  Each
 *                                enqueue slot keeps a device workspace of (resident workgroups) x (level size padded to 256)
 *                                x 4 bytes for the largest active level: 0.63 GB for 640x480 on 512 workgroups; it is
 *                                kept until the engine is destroyed, also under another objective.
 *                                phovo_engine_enqueue_align_prior, the six phovo_engine_evaluate_* calls and their
 *                                phovo_odometry_get_*_system calls are PHOVO_E_UNSUPPORTED under this objective.  Fusion,
 *                                sliding-window, wide, latency-form and batch-invariant settings are accepted and have no
 *                                effect. */
#define PHOVO_OBJECTIVE_INVERSE_SEMIDENSE 7

/* Option of the semi-dense inverse-compositional objective: tau_L, the smallest gradient magnitude (of the stored gradient
 * planes) a selected pixel has on level L.  The default, 0 everywhere, selects every depth-valid pixel with finite
 * gradients. */
typedef struct phovo_semidense_options {
  double min_pixel_gradient[PHOVO_MAX_LEVELS];  /* finite and >= 0 */
} phovo_semidense_options;

/* Per pair and level: the selected pixels (levels with max_num_iterations 0 stay 0). */
typedef struct phovo_semidense_report {
  int32_t selected[PHOVO_MAX_LEVELS];
} phovo_semidense_report;

/* Option of the robust inverse-compositional objective: delta = scale_factor * (median of |r|).  The default,
 * 1.345 * 1.4826, is Huber's 95 %-efficiency constant times the factor that makes the median absolute deviation a
 * consistent estimate of a normal sigma. */
typedef struct phovo_robust_options {
  double scale_factor;                          /* finite and > 0 */
} phovo_robust_options;

/* Per pair and level, from the level's LAST system (levels with max_num_iterations 0 stay 0). */
typedef struct phovo_robust_report {
  double  delta[PHOVO_MAX_LEVELS];              /* the Huber threshold that system was built with */
  int32_t outliers[PHOVO_MAX_LEVELS];           /* its rows with fabs(r) > delta */
} phovo_robust_report;

/* The weighted Gauss-Newton system of one frame pair under the robust inverse-compositional objective at a given state on
 * one level (phovo_engine_evaluate_robust_pairs, which has the contract; phovo_odometry_get_robust_system). */
typedef struct phovo_robust_system {
  double   information[36];  /* sum w J J^T, twist basis (nu, omega) of T Exp(xi), row-major, exactly symmetric */
  double   gradient[6];      /* sum w J r */
  double   cost;             /* sum w r^2            (r^T W r, as phovo_pair_system.cost under a Huber weight) */
  double   huber_cost;       /* sum (|r| <= delta ? r^2 : 2 delta |r| - delta^2)   = 2 sum rho_delta(r) */
  double   squared_cost;     /* sum r^2 */
  double   delta;            /* the threshold the weights were built with */
  double   median;           /* m of the median rule at this state; 0 when deltas were given */
  int32_t  rows, outliers;   /* rows as valid_pixels counts them; rows with fabs(r) > delta */
  uint32_t flags;            /* PHOVO_PAIR_RANK_DEFICIENT if rows < 6; PHOVO_PAIR_NONFINITE if any sum is inf/NaN */
  int32_t  reserved;         /* 0 */
} phovo_robust_system;

/* A Gaussian pose prior for objectives 5 and 6 (phovo_engine_enqueue_align_prior, phovo_odometry_set_pose_prior; not in the
 * reference; DESIGN.md §24 has the contract).  Each pair gets a prior pose, a state (x, y, z, yaw, pitch, roll) with
 * T_p = eigenPose(state) = (R_p, t_p), and a symmetric 6 x 6 information matrix Lambda in the twist order (nu, omega) of the
 * right-hand perturbation T Exp(xi) -- the basis phovo_engine_evaluate_inverse_pairs returns.  Each level L has a scale s_L
 * (phovo_prior_options.level_scale).  In every iteration, before the solve, with the level's current (R, t):
 *     e   = Log(T_p^-1 T) = Log(R_p^T R, R_p^T (t - t_p)), a twist;
 *     H'  = H + s_L Lambda,   g' = g + s_L Lambda e;
 *     xi  = -lambda_L H'^-1 g', composed as without a prior.
 * The prior's Jacobian is taken as the identity (first order in e, as in Kerl et al.'s dense RGB-D odometry): the fixed
 * point satisfies g + s_L Lambda e = 0, not the exact stationarity condition with the right Jacobian of Log.  Termination and
 * the reported gradient_norm use ||g'||_2.  PHOVO_PAIR_RANK_DEFICIENT keeps its meaning (a system with fewer than 6 data
 * rows, sticky); the pose may now be finite beside it.  Under objective 6, H and g are the weighted sums; the median, delta
 * and the outlier count do not see the prior.
 *   Log(R, t):  w = vee(R - R^T) / 2, s = |w|, c = (tr R - 1) / 2, th = atan2(s, c), omega = (th / s) w,
 *               nu = (I - W / 2 + D W^2) t with W = [omega]x and D = (1 - (th / 2) cot(th / 2)) / th^2; below th^2 = 1e-8
 *               th / s = 1 + th^2 / 6 + 7 th^4 / 360 and D = 1 / 12 + th^2 / 720 + th^4 / 30240.  Relative rotations beyond
 *               3.0 rad between prior and pose are outside the accuracy contract; the result is finite wherever s != 0.
 * With Lambda = 0, or s_L = 0, the two additions are skipped and every output bit equals the call without a prior. */
typedef struct phovo_prior_options {
  double level_scale[PHOVO_MAX_LEVELS];         /* s_L: finite and >= 0; default 1 on every level */
} phovo_prior_options;

/* Per pair, at the pose the finest executed level ended on (all 0 when no level ran). */
typedef struct phovo_prior_report {
  double error[6];                              /* e = Log(T_p^-1 T), twist order (nu, omega) */
  double prior_cost;                            /* e^T Lambda e (without s_L); 0 where Lambda = 0 */
} phovo_prior_report;

/* Options of the photometric-geometric objective, per level.  Both are settings to tune for the sensor and the scene, not
 * measured optima: depth_weight trades metres of depth error against intensity error (intensities are in [0, 1]), and
 * max_depth_residual is the occlusion gate -- without one, depth rows across a depth discontinuity pull the pose away
 * (DESIGN.md §16). */
typedef struct phovo_geometric_options {
  double depth_weight[PHOVO_MAX_LEVELS];        /* sigma_L: finite and > 0.  yml: "depth_weight (at each level)"          */
  double max_depth_residual[PHOVO_MAX_LEVELS];  /* metres; <= 0 switches the gate off.  yml: "max_depth_residual (at each level)" */
} phovo_geometric_options;

/* Per pair and level, from the level's LAST system (levels with max_num_iterations 0 stay 0). */
typedef struct phovo_geometric_report {
  int32_t depth_rows[PHOVO_MAX_LEVELS];         /* depth rows (phovo_pair_report.valid_pixels has the photometric rows) */
  double  photometric_cost[PHOVO_MAX_LEVELS];   /* sum r_I^2 */
  double  depth_cost[PHOVO_MAX_LEVELS];         /* sum r_D^2 (sigma_L included) */
} phovo_geometric_report;

/* The Gauss-Newton system of one frame pair under the photometric-geometric objective at a given state on one level
 * (phovo_engine_evaluate_geometric_pairs, phovo_odometry_get_geometric_system), with the photometric and
 * the depth block kept apart.  Its rows are the ones gn_level_kernel_geometric fills at that state: the photometric rows
 * are the bilinear extension's with the true warp Jacobian, and a depth row sits beside a photometric row iff the four
 * clamped taps of the target's depth pass min_depth < d < max_depth (NaN fails) and, with max_depth_residual[level] > 0,
 * |D1(u, v) - Z'| <= max_depth_residual[level].  sigma and the gate are the engine's phovo_geometric_options at that
 * level.  The gate acts on the UNWEIGHTED residual, so the system under another weight sigma' is
 * photometric_information + (sigma'/sigma)^2 depth_information (gradient and cost likewise) without another pass.
 * Relation to the aligner: the system it solves in iteration k of a level is information / gradient at the state the
 * iteration starts from.  The photometric block is bit for bit the phovo_sampled_system that
 * phovo_engine_evaluate_sampled_pairs returns for the same pool and state under the photometric objective with
 * PHOVO_SAMPLING_BILINEAR and jacobian_corrected = 1.  Arithmetic: fp64 on the device; the sums are taken in an order that
 * depends on the level size only, so a pair's result is the same bit for bit whatever the batch, its position in it, or
 * the engine's settings. */
typedef struct phovo_geometric_system {
  double   information[36];              /* photometric_information + depth_information, entry by entry, ONE fp64 add each */
  double   gradient[6];                  /* photometric_gradient + depth_gradient, likewise */
  double   photometric_information[36];  /* sum J_I J_I^T, row-major, exactly symmetric (filled from the upper triangle) */
  double   photometric_gradient[6];      /* sum J_I r_I */
  double   depth_information[36];        /* sum J_D J_D^T, sigma_L included */
  double   depth_gradient[6];            /* sum J_D r_D */
  double   photometric_cost;             /* sum r_I^2 */
  double   depth_cost;                   /* sum r_D^2 (sigma_L included) */
  int32_t  rows, depth_rows;             /* as phovo_pair_report.valid_pixels / phovo_geometric_report.depth_rows count them */
  uint32_t flags;                        /* PHOVO_PAIR_RANK_DEFICIENT if rows < 6; PHOVO_PAIR_NONFINITE if any sum of either block is inf/NaN */
  int32_t  reserved;
} phovo_geometric_system;

/* Solver options of the trust-region objective, per level (CPhotoconsistencyOdometryCeres.h:526-576).  num_levels, blur,
 * gradient scale and max_num_iterations stay in phovo_config. */
typedef struct phovo_trust_region_options {
  double function_tolerance[PHOVO_MAX_LEVELS];          /* function_tolerance (at each level)           */
  double gradient_tolerance[PHOVO_MAX_LEVELS];          /* gradient_tolerance (at each level)           */
  double parameter_tolerance[PHOVO_MAX_LEVELS];         /* parameter_tolerance (at each level)          */
  double initial_trust_region_radius[PHOVO_MAX_LEVELS]; /* initial_trust_region_radius (at each level)  */
  double max_trust_region_radius[PHOVO_MAX_LEVELS];     /* max_trust_region_radius (at each level)      */
  double min_trust_region_radius[PHOVO_MAX_LEVELS];     /* min_trust_region_radius (at each level)      */
  double min_relative_decrease[PHOVO_MAX_LEVELS];       /* min_relative_decrease (at each level)        */
} phovo_trust_region_options;

/* Why a level of the trust-region solver stopped (phovo_trust_region_level.termination). */
#define PHOVO_TR_SKIPPED           0   /* max_num_iterations[L] == 0: the level was not optimised             */
#define PHOVO_TR_MAX_ITERATIONS    1   /* NO_CONVERGENCE: max_num_iterations steps taken                        */
#define PHOVO_TR_GRADIENT          2   /* CONVERGENCE: max |x - (x - g)| <= gradient_tolerance                   */
#define PHOVO_TR_FUNCTION          3   /* CONVERGENCE: |cost change| <= function_tolerance * cost               */
#define PHOVO_TR_PARAMETER         4   /* CONVERGENCE: |step| <= parameter_tolerance * (|x| + parameter_tolerance) */
#define PHOVO_TR_MIN_RADIUS        5   /* CONVERGENCE: radius <= min_trust_region_radius                        */
#define PHOVO_TR_INVALID_STEP      6   /* FAILURE: the LM system could not be solved or did not promise a decrease */
#define PHOVO_TR_EVALUATION_FAILED 7   /* FAILURE: the cost or the system at the point was not finite           */
typedef struct phovo_trust_region_level {
  int32_t steps;          /* LM steps (iteration 0, the first evaluation, not counted)      */
  int32_t accepted;       /* steps whose candidate was accepted                              */
  int32_t termination;    /* PHOVO_TR_*                                                      */
  int32_t rows;           /* owned targets (filled rows) at the final point                 */
  double  initial_cost;   /* 1/2 sum r^2 at the level's first point                          */
  double  final_cost;     /* at the level's final point (the last accepted one)              */
  double  final_radius;   /* the trust-region radius when the level stopped                  */
  double  jacobi_scaling[6]; /* S_j = 1 / (1 + sqrt(H_jj)) from the level's first system (0 if it failed) */
} phovo_trust_region_level;
typedef struct phovo_trust_region_report {
  phovo_trust_region_level level[PHOVO_MAX_LEVELS];
} phovo_trust_region_report;

typedef struct phovo_engine phovo_engine;
typedef struct phovo_odometry phovo_odometry;

/* ---- library ---------------------------------------------------------------------------- */
const char *phovo_version(void);
const char *phovo_status_string(int status);
/* Message of the most recent failure on the calling thread ("" if none). */
const char *phovo_last_error(void);
/* Number of HIP devices visible (0 if none / no driver). */
int phovo_device_count(void);

/* ---- configuration: ...Analytic.h:430-443 (defaults), :581-607 (ReadConfigurationFile) ---- */
int phovo_config_default(phovo_config *cfg);
/* Parses the reference's config_files/ *.yml unchanged (OpenCV FileStorage "%YAML:1.0" dialect,
 * keys with spaces and parentheses, per-level arrays that may be longer than num_levels). */
int phovo_config_read_file(const char *path, phovo_config *cfg);

/* The trust-region objective's keys (CPhotoconsistencyOdometryCeres.h:526-576): numOptimizationLevels, blurFilterSize,
 * imageGradientsScalingFactor, max_num_iterations into cfg (lambda and min_gradient_norm keep their defaults) and the
 * seven solver lists into opt; num_threads, num_linear_solver_threads, minimizer_progress_to_stdout and
 * visualizeIterations are read and ignored (cfg->visualize_iterations is 0).  Lists may be longer than
 * numOptimizationLevels.  A min_trust_region_radius list one entry short takes Ceres's default 1e-32 for the missing last
 * (coarsest) level, as 4 of the reference's 8 files need; any other short list or missing key is PHOVO_E_CONFIG (so is an
 * analytic file).  cfg or opt may be NULL. */
int phovo_trust_region_read_file(const char *path, phovo_config *cfg, phovo_trust_region_options *opt);
/* Ceres's defaults for every level: function 1e-6, gradient 1e-10, parameter 1e-8, radius 1e4 (max 1e16, min 1e-32),
 * min_relative_decrease 1e-3. */
int phovo_trust_region_options_default(phovo_trust_region_options *opt);

/* Photometric-geometric objective: depth_weight 1.0 and max_depth_residual 0.1 m on every level (starting points, not
 * measured optima). */
int phovo_geometric_options_default(phovo_geometric_options *opt);
/* The two optional keys of an ANALYTIC yml file, "depth_weight (at each level): [..]" and "max_depth_residual (at each
 * level): [..]" (the reference's loader ignores keys it does not ask for, as it does the extension keys).  An absent key
 * leaves the defaults; a list shorter than the file's numOptimizationLevels (where the file has that key), a malformed one
 * or a weight that is not finite and > 0 is PHOVO_E_CONFIG.  The rest of the file is not read: phovo_config_read_file. */
int phovo_geometric_read_file(const char *path, phovo_geometric_options *opt);

/* Robust inverse-compositional objective: scale_factor 1.345 * 1.4826. */
int phovo_robust_options_default(phovo_robust_options *opt);

/* Semi-dense inverse-compositional objective: min_pixel_gradient 0 on every level (every depth-valid pixel). */
int phovo_semidense_options_default(phovo_semidense_options *opt);
/* The optional key of an ANALYTIC yml file, "min_pixel_gradient (at each level): [..]", read the way
 * phovo_geometric_read_file reads depth_weight: an absent key leaves the defaults; a list shorter than the file's
 * numOptimizationLevels, a malformed one or a value that is not finite and >= 0 is PHOVO_E_CONFIG. */
int phovo_semidense_read_file(const char *path, phovo_semidense_options *opt);

int phovo_extensions_default(phovo_extensions *ext);
/* Optional keys in the same yml file (the reference's cv::FileStorage lookups ignore keys they do not ask for,
 * so such a file still loads there): "huber_delta (at each level): [..]", "plane_storage_bits: 64|32|16",
 * "sampling_bilinear: 0|1", "jacobian_corrected: 0|1".
 * Absent keys leave the defaults (everything off). */
int phovo_extensions_read_file(const char *path, phovo_extensions *ext);

/* eigenPose, CPhotoconsistencyOdometry.h:47-71: (x,y,z,yaw,pitch,roll) -> row-major 4x4. */
int phovo_eigen_pose(const double state[6], double rt[16]);
/* The inverse of phovo_eigen_pose (host arithmetic only): state = (rt[3], rt[7], rt[11], yaw = atan2(R10, R00),
 * pitch = atan2(-R20, sqrt(R00^2 + R10^2)), roll = atan2(R21, R22)) of a row-major 4x4 -- the formulas by which the
 * inverse-compositional objective leaves a level.  Exact up to rounding wherever cos(pitch) != 0 (pitch comes back in
 * [-pi/2, pi/2]; at cos(pitch) = 0 yaw and roll are not determined by the matrix).  PHOVO_E_INVALID_ARGUMENT on NULL. */
int phovo_state_from_pose(const double rt[16], double state[6]);

/* The VisualOdometry app's pose chain and trajectory line
 * (apps/PhotoconsistencyVisualOdometry/PhotoconsistencyVisualOdometry.cpp:233-243):
 *   pose *= Rt^-1 per pair, starting from `pose_io` (row-major 4x4; identity at the start of a sequence), with
 *   Rt = eigenPose(states[p]); poses_out[p] (may be NULL) receives the pose after pair p, pose_io the last one.
 * Host arithmetic only (no GPU): one implementation shared by the app's loop, its --batch path and the sharded
 * sequence driver, so that their trajectory files are byte-identical. */
int phovo_trajectory_chain(int n_pairs, const double *states /* [n_pairs][6] */, double pose_io[16],
                           double *poses_out /* [n_pairs][16] or NULL */);
/* `timestamp tx ty tz qx qy qz qw` with digits10 + 1 = 16 significant digits (:240-243), quaternion from the
 * rotation block as Eigen::Quaternion(Matrix3) builds it (:237); no newline.  Returns PHOVO_E_INVALID_ARGUMENT if
 * `capacity` is too small (256 always suffices). */
int phovo_trajectory_format_pose(double timestamp, const double pose[16], char *line, size_t capacity);
/* One line of the VisualOdometry app's --information file: `timestamp rows cost` and the 21 upper-triangle entries of
 * s->information in row-major order (H00 H01 .. H05 H11 .. H55), every double as "%.17g" (round-trips exactly), no
 * newline.  Host only.  PHOVO_E_INVALID_ARGUMENT for NULL pointers or if `capacity` is too small (640 always suffices). */
int phovo_pair_system_format(double timestamp, const phovo_pair_system *s, char *line, size_t capacity);
/* One line of the VisualOdometry app's --robust-system file: `timestamp rows outliers delta median cost huber_cost
 * squared_cost`, the 6 entries of s->gradient and the 21 upper-triangle entries of s->information in row-major order, every
 * double as "%.17g" (round-trips exactly), no newline.  Host only.  PHOVO_E_INVALID_ARGUMENT for NULL pointers or if
 * `capacity` is too small (1024 always suffices: 33 doubles of at most 24 characters, two integers, 34 blanks). */
int phovo_robust_system_format(double timestamp, const phovo_robust_system *s, char *line, size_t capacity);
/* One line for a phovo_prior_report: `timestamp prior_cost` and the 6 entries of r->error, every double as "%.17g"
 * (round-trips exactly), no newline.  Host only.  PHOVO_E_INVALID_ARGUMENT for NULL pointers or if `capacity` is too small
 * (256 always suffices). */
int phovo_prior_report_format(double timestamp, const phovo_prior_report *r, char *line, size_t capacity);

/* One line of the VisualOdometry app's --system file: `timestamp rows cost dim` and the dim (dim + 1) / 2 upper-triangle
 * entries of s->information in row-major order, every double as "%.17g" (round-trips exactly), no newline.  Host only.
 * PHOVO_E_INVALID_ARGUMENT for NULL pointers, a dim that is neither 6 nor 8, or if `capacity` is too small (1024 always
 * suffices). */
int phovo_sampled_system_format(double timestamp, const phovo_sampled_system *s, char *line, size_t capacity);

/* One line of the VisualOdometry app's --geometric-system file: `timestamp rows depth_rows photometric_cost depth_cost`,
 * the 21 upper-triangle entries of s->photometric_information in row-major order, then the 21 of s->depth_information;
 * every double as "%.17g" (round-trips exactly), no newline.  A reader recovers s->information bit for bit with the one
 * add per entry that built it.  Host only.  PHOVO_E_INVALID_ARGUMENT for NULL pointers or a `capacity` below
 * PHOVO_GEOMETRIC_SYSTEM_LINE_CAPACITY, which always suffices: 45 doubles of at most 24 characters, two integers of at most
 * 11, 46 blanks and the terminator are 1149 bytes. */
#define PHOVO_GEOMETRIC_SYSTEM_LINE_CAPACITY 1280
int phovo_geometric_system_format(double timestamp, const phovo_geometric_system *s, char *line, size_t capacity);

/* warpImage, CPhotoconsistencyOdometry.h:73-134 -- the forward warp both reference apps call after Optimize()
 * (...FrameAlignment.cpp:108, ...VisualOdometry.cpp:248-250) to show |I1 - warp(I0)|.  Host buffers in and out,
 * strides in bytes; rt row-major 4x4, k row-major 3x3, level scales the intrinsics by 2^-level as the reference does.
 * Reference semantics: depth > 0 gate, truncating cast of the projected position, the last source pixel in raster
 * order that lands on a target pixel stays, zeros elsewhere. */
int phovo_warp_image(int device, const uint8_t *intensity, size_t intensity_stride_bytes,
                     const double *depth, size_t depth_stride_bytes, int w, int h, const double rt[16],
                     const double k[9], int level, uint8_t *warped, size_t warped_stride_bytes);

/* ---- single pair: 1:1 with CPhotoconsistencyOdometryAnalytic<unsigned char,double> ------- */
int phovo_odometry_create(int device, phovo_odometry **out);               /* ctor  :430-443 */
int phovo_odometry_destroy(phovo_odometry *o);                             /* dtor  :445     */
int phovo_odometry_read_configuration_file(phovo_odometry *o, const char *path);   /* :581 */
int phovo_odometry_set_config(phovo_odometry *o, const phovo_config *cfg);
int phovo_odometry_set_extensions(phovo_odometry *o, const phovo_extensions *ext);   /* not in the reference */
/* not in the reference: 1 = Optimize() may take the forms that finish soonest for ONE pair (phovo_engine_set_latency_forms:
 * last bits may then differ from the same pair aligned in a batch); default 0 */
int phovo_odometry_set_latency_forms(phovo_odometry *o, int on);
/* not in the reference's class (its apps pick the class): PHOVO_OBJECTIVE_*, default photometric.  A change drops the
 * frames set so far.  Under the bi-objective phovo_odometry_set_target_frame needs depth (NULL: PHOVO_E_INVALID_ARGUMENT). */
int phovo_odometry_set_objective(phovo_odometry *o, int objective);
/* Trust-region objective: its solver options (defaults: phovo_trust_region_options_default) and the solver record of the
 * last Optimize() (PHOVO_E_NOT_READY before one; PHOVO_E_UNSUPPORTED under another objective).  Under this objective
 * phovo_odometry_read_configuration_file reads the Ceres keys (phovo_trust_region_read_file). */
int phovo_odometry_set_trust_region_options(phovo_odometry *o, const phovo_trust_region_options *opt);
int phovo_odometry_get_trust_region_options(const phovo_odometry *o, phovo_trust_region_options *opt);
int phovo_odometry_get_trust_region_report(const phovo_odometry *o, phovo_trust_region_report *report);
/* Affine-illumination objective: (alpha, beta) of the last Optimize() (PHOVO_E_NOT_READY before a successful one;
 * PHOVO_E_UNSUPPORTED under another objective).  The target's intensities are modelled as (1 + alpha) I0 + beta. */
int phovo_odometry_get_illumination(const phovo_odometry *o, double alpha_beta[2]);
/* Photometric-geometric objective: its options (defaults: phovo_geometric_options_default; kept under every objective,
 * used by this one; a weight that is not finite and > 0 is PHOVO_E_INVALID_ARGUMENT) and the record of the last Optimize()
 * (PHOVO_E_NOT_READY before a successful one; PHOVO_E_UNSUPPORTED under another objective).  Under this objective
 * phovo_odometry_set_target_frame needs depth (NULL: PHOVO_E_INVALID_ARGUMENT) and uploads the target with both roles, and
 * phovo_odometry_read_configuration_file reads the two optional keys as well (phovo_geometric_read_file). */
int phovo_odometry_set_geometric_options(phovo_odometry *o, const phovo_geometric_options *opt);
int phovo_odometry_get_geometric_options(const phovo_odometry *o, phovo_geometric_options *opt);
int phovo_odometry_get_geometric_report(const phovo_odometry *o, phovo_geometric_report *report);
/* Robust inverse-compositional objective: its options (default: phovo_robust_options_default; kept under every objective,
 * used by this one; a scale_factor that is not finite and > 0 is PHOVO_E_INVALID_ARGUMENT) and the record of the last
 * Optimize() (PHOVO_E_NOT_READY before a successful one; PHOVO_E_UNSUPPORTED under another objective).  Under this
 * objective phovo_odometry_set_source_frame uploads the source with both roles, as under objective 5. */
int phovo_odometry_set_robust_options(phovo_odometry *o, const phovo_robust_options *opt);
int phovo_odometry_get_robust_options(const phovo_odometry *o, phovo_robust_options *opt);
int phovo_odometry_get_robust_report(const phovo_odometry *o, phovo_robust_report *report);
/* Semi-dense inverse-compositional objective: its options (default: phovo_semidense_options_default; kept under every
 * objective, used by this one; a min_pixel_gradient that is not finite and >= 0 is PHOVO_E_INVALID_ARGUMENT) and the record
 * of the last Optimize() (PHOVO_E_NOT_READY before a successful one; PHOVO_E_UNSUPPORTED under another objective).  Under
 * this objective phovo_odometry_set_source_frame uploads the source with both roles, as under objective 5, and
 * phovo_odometry_read_configuration_file reads the optional key as well (phovo_semidense_read_file). */
int phovo_odometry_set_semidense_options(phovo_odometry *o, const phovo_semidense_options *opt);
int phovo_odometry_get_semidense_options(const phovo_odometry *o, phovo_semidense_options *opt);
int phovo_odometry_get_semidense_report(const phovo_odometry *o, phovo_semidense_report *report);
/* Gaussian pose prior (phovo_prior_options above has the rule): the prior of every later Optimize() until it is cleared or
 * set again -- state[6] the prior pose, information[36] row-major with its upper triangle read; a non-finite entry or a
 * negative diagonal is PHOVO_E_INVALID_ARGUMENT.  It may be set under any objective; Optimize() with a prior set is
 * PHOVO_E_UNSUPPORTED under any objective but 5 and 6.  The level scales (default 1; kept under every objective) and the
 * record of the last Optimize() (PHOVO_E_NOT_READY before a successful one; PHOVO_E_UNSUPPORTED if it ran without a prior). */
int phovo_odometry_set_pose_prior(phovo_odometry *o, const double state[6], const double information[36]);
int phovo_odometry_clear_pose_prior(phovo_odometry *o);
int phovo_odometry_set_prior_options(phovo_odometry *o, const phovo_prior_options *opt);
int phovo_odometry_get_prior_options(const phovo_odometry *o, phovo_prior_options *opt);
int phovo_odometry_get_prior_report(const phovo_odometry *o, phovo_prior_report *report);
int phovo_odometry_set_min_depth(phovo_odometry *o, double min_depth);     /* :448 */
int phovo_odometry_set_max_depth(phovo_odometry *o, double max_depth);     /* :454 */
int phovo_odometry_set_intrinsic_matrix(phovo_odometry *o, const double k[9]);     /* :460, row-major 3x3 */
/* SetSourceFrame :466-476 -- intensity u8, depth fp64 metres; builds the intensity and depth pyramids. */
int phovo_odometry_set_source_frame(phovo_odometry *o,
                                    const uint8_t *intensity, size_t intensity_stride,
                                    const double *depth, size_t depth_stride,
                                    int width, int height);
/* SetTargetFrame :479-491 -- depth is ignored (may be NULL); builds intensity + Scharr pyramids. */
int phovo_odometry_set_target_frame(phovo_odometry *o,
                                    const uint8_t *intensity, size_t intensity_stride,
                                    const double *depth, size_t depth_stride,
                                    int width, int height);
int phovo_odometry_set_initial_state_vector(phovo_odometry *o, const double state[6]);     /* :494 */
int phovo_odometry_optimize(phovo_odometry *o);                                            /* :500 */
int phovo_odometry_get_optimal_state_vector(const phovo_odometry *o, double state[6]);     /* :566 */
int phovo_odometry_get_optimal_rigid_transformation_matrix(const phovo_odometry *o, double rt[16]); /* :572 */
int phovo_odometry_get_report(const phovo_odometry *o, phovo_pair_report *report);
/* not in the reference: the system (phovo_pair_system) at the optimal state on the finest level the configuration
 * optimises (the lowest L with max_num_iterations[L] > 0), evaluated on demand (Optimize() and its timing are unchanged).
 * PHOVO_E_NOT_READY before a successful Optimize() and after a Set*Frame since; PHOVO_E_UNSUPPORTED as for
 * phovo_engine_evaluate_pairs (bilinear sampling, bi-objective). */
int phovo_odometry_get_pair_system(const phovo_odometry *o, phovo_pair_system *out);
/* not in the reference: the system (phovo_sampled_system) of the sampled aligners at the optimal state on the finest
 * level the configuration optimises, evaluated on demand; under the affine objective at the (alpha, beta) of the last
 * Optimize().  PHOVO_E_NOT_READY before a successful Optimize() and after a Set*Frame since; PHOVO_E_UNSUPPORTED as for
 * phovo_engine_evaluate_sampled_pairs (nearest / scatter sampling, bi-objective, trust region). */
int phovo_odometry_get_sampled_system(const phovo_odometry *o, phovo_sampled_system *out);
/* not in the reference: the system (phovo_geometric_system) of the photometric-geometric objective at the optimal state
 * on the finest level the configuration optimises, evaluated on demand.  PHOVO_E_NOT_READY before a successful Optimize()
 * and after a Set*Frame since; PHOVO_E_UNSUPPORTED under another objective. */
int phovo_odometry_get_geometric_system(const phovo_odometry *o, phovo_geometric_system *out);
/* not in the reference: the system (phovo_pair_system) of the trust-region and of the bi-objective objective at the
 * optimal state on the finest level the configuration optimises, evaluated on demand
 * (phovo_engine_evaluate_objective_pairs).  PHOVO_E_UNSUPPORTED under any other objective; PHOVO_E_NOT_READY before a
 * successful Optimize() and after a Set*Frame since. */
int phovo_odometry_get_objective_system(const phovo_odometry *o, phovo_pair_system *out);
/* not in the reference: the twist-basis system (phovo_pair_system) of the inverse-compositional objective at the optimal
 * state on the finest level the configuration optimises, evaluated on demand (phovo_engine_evaluate_inverse_pairs has the
 * contract: a right-hand twist in the source camera's frame).  PHOVO_E_UNSUPPORTED under any other objective;
 * PHOVO_E_NOT_READY before a successful Optimize() and after a Set*Frame since. */
int phovo_odometry_get_inverse_system(const phovo_odometry *o, phovo_pair_system *out);
/* not in the reference: the weighted twist-basis system (phovo_robust_system) of the robust inverse-compositional
 * objective at the optimal state on the finest level the configuration optimises, with the median rule taken at that state
 * (phovo_engine_evaluate_robust_pairs with deltas == NULL has the contract), evaluated on demand.  PHOVO_E_UNSUPPORTED under
 * any other objective; PHOVO_E_NOT_READY before a successful Optimize() and after a Set*Frame since. */
int phovo_odometry_get_robust_system(const phovo_odometry *o, phovo_robust_system *out);
/* Device time of the last Optimize() in milliseconds (HIP events; the reference wraps the same
 * call in cv::TickMeter, apps/PhotoconsistencyFrameAlignment/PhotoconsistencyFrameAlignment.cpp:99-102). */
int phovo_odometry_last_optimize_ms(const phovo_odometry *o, double *ms);

/* ---- batched engine ------------------------------------------------------------------------ */
#define PHOVO_ROLE_SOURCE 1   /* needs intensity + depth pyramids   (SetSourceFrame) */
#define PHOVO_ROLE_TARGET 2   /* needs intensity + gradient pyramids (SetTargetFrame) */
#define PHOVO_ROLE_BOTH   3

int phovo_engine_create(int device, phovo_engine **out);
int phovo_engine_destroy(phovo_engine *e);
int phovo_engine_set_config(phovo_engine *e, const phovo_config *cfg);
int phovo_engine_get_config(const phovo_engine *e, phovo_config *cfg);
/* Changing plane_storage drops the frame pool (like a configuration that changes the levels).  So does changing `sampling`
 * while plane_storage is PHOVO_STORAGE_F16 (before and after the call): fp16 planes carry bilinear tap records exactly under
 * PHOVO_SAMPLING_BILINEAR, and the pool is laid out with or without them.  The call still returns PHOVO_OK; the frames are
 * gone, and the next align / evaluate is refused with PHOVO_E_NOT_READY until phovo_engine_reserve_frames and the uploads
 * have been repeated.  Every other change (Huber deltas, jacobian_corrected, sampling on fp64 / fp32 planes) keeps the
 * resident frames.
 * Precondition of PHOVO_SAMPLING_BILINEAR on PHOVO_STORAGE_F64 planes, for levels ONE COLUMN wide (width >> level == 1) only:
 * all four planes of a target frame must be finite on that level, its depth included when the frame was uploaded with
 * PHOVO_ROLE_BOTH or given a depth plane.  The fp64 kernel loads a row's two taps as one 16-byte pair and weights the
 * second, which on a one-column row is the double stored behind the row, by zero: a NaN there (an invalid-depth marker)
 * makes the sample NaN and the pair ends PHOVO_PAIR_NONFINITE.  The fp32 and fp16 storages clamp their taps and carry no
 * such condition; nor do levels two or more columns wide on any storage. */
int phovo_engine_set_extensions(phovo_engine *e, const phovo_extensions *ext);
int phovo_engine_get_extensions(const phovo_engine *e, phovo_extensions *ext);
int phovo_engine_set_intrinsic_matrix(phovo_engine *e, const double k[9]);
int phovo_engine_set_depth_range(phovo_engine *e, double min_depth, double max_depth);
/* 0 (default): only levels with max_num_iterations > 0 are built and kept in HBM (the others are
 * never read by Optimize()).  1: every level, as the reference does (:474-475,487-490). */
int phovo_engine_set_build_all_levels(phovo_engine *e, int on);

/* How a level is run.  The persistent form gives every pair ONE workgroup for all iterations of a level (the
 * throughput form).  The wide form cuts a pair into tiles of 1024 pixels, one workgroup each, with two launches
 * per iteration and a host look at the "done" words every 8 iterations (the latency form for a handful of pairs on
 * a large level; reference-exact configuration only).  policy: 0 = automatic, 1 = wide wherever possible, -1 = never.
 * Automatic: wide iff n_pairs <= 32 and the level's owner map does not fit LDS (more than ~39 k pixels: 320x240,
 * 640x480 -- one workgroup would need hundreds of microseconds per iteration there); never with
 * phovo_engine_set_batch_invariant.  Same iteration counts and poses within the parity bar either way (the forms sum in
 * different orders). */
int phovo_engine_set_wide_policy(phovo_engine *e, int policy);
/* Levels whose owner map exceeds LDS (more than ~39 k pixels) run the sliding-window kernel (owner ring in LDS) followed
 * by the exact kernel (owner map in HBM) for the pairs whose warp left the window.  policy: 0 = automatic (that), -1 =
 * exact kernel only.  Results are the same either way (tests/test_gpu_parity.py). */
int phovo_engine_set_slide_policy(phovo_engine *e, int policy);
/* Consecutive pyramid levels in ONE launch.  The reference's Optimize() loops per pair over levels
 * (CPhotoconsistencyOdometryAnalytic.h:502-563); with a gradient threshold (min_gradient_norm > 0, :388) a pair leaves a
 * level after a data-dependent number of iterations, and one launch per level would make every level boundary a boundary
 * for the whole batch.  PHOVO_FUSION_AUTO (default): where two or more consecutive active levels each fit the 512-thread
 * scatter kernel with its owner map in half a CU's LDS (more than 2048 and up to 19 328 pixels: 80x60 and 160x120 of
 * a 640x480 pyramid) and at least one of them has a gradient threshold, those levels are one persistent launch in which a
 * workgroup runs a pair through all of them back to back.  PHOVO_FUSION_OFF: one launch per level, each in the geometry
 * that suits it alone (what a configuration without thresholds gets anyway).  PHOVO_FUSION_SPLIT: one launch per level in
 * the geometry of the fused launch -- bit-identical to PHOVO_FUSION_AUTO, for tests.  Iteration counts are the same in all
 * three; poses agree to the parity bar between AUTO and OFF (other summation order on the smaller levels). */
enum { PHOVO_FUSION_AUTO = 0, PHOVO_FUSION_OFF = -1, PHOVO_FUSION_SPLIT = -2 };
int phovo_engine_set_level_fusion(phovo_engine *e, int mode);
/* One arithmetic per pair.  The reference has one (CPhotoconsistencyOdometryAnalytic.h:500-563), and so has this library
 * wherever it costs little: on every level whose owner map fits LDS (up to ~39 k pixels -- every active level of the
 * shipped 4- and 5-level files on 640x480) a pair runs the SAME kernel in the same geometry whether it is aligned alone
 * through phovo_odometry_optimize or as one of thousands in a batch, so its state vector is the same bit for bit
 * (PhotoconsistencyVisualOdometry: the pair-by-pair loop and --batch write the same file).  Two switches move that line:
 *   phovo_engine_set_latency_forms(e, 1)   a handful of pairs (<= 8 / <= 32) may take the forms that finish soonest on
 *       those levels too: 512-thread workgroups for levels of <= 9.5 k pixels, the wide form from 16 384 pixels (160x120:
 *       12 instead of 27 us per iteration).  Same iteration counts, poses within the parity bar of the batch forms, last
 *       bits may differ.  Default 0.
 *   phovo_engine_set_batch_invariant(e, 1) also levels ABOVE ~39 k pixels take the batch forms for every batch size (no
 *       automatic wide form), so that a sequence cut into shards of any sizes gives bit-identical poses on every
 *       configuration.  What the sequence drivers set (apps/PhotoconsistencyVisualOdometry --batch, sequence.py,
 *       bench.py).  Default 0: one pair on 640x480 level 0 takes 22 us per iteration in the wide form, 520 us in one
 *       workgroup. */
int phovo_engine_set_latency_forms(phovo_engine *e, int on);
int phovo_engine_set_batch_invariant(phovo_engine *e, int on);
/* 1 if `level` would run in the wide form for a batch of n_pairs under the current settings. */
int phovo_engine_level_uses_wide(const phovo_engine *e, int level, int n_pairs);
/* PHOVO_OBJECTIVE_*.  A change of objective drops the frame pool (as a change of plane_storage does): reserve_frames
 * and upload again.  PHOVO_E_UNSUPPORTED for the bi-objective under anything but fp64 planes, nearest / scatter
 * sampling and no Huber weights. */
int phovo_engine_set_objective(phovo_engine *e, int objective);
int phovo_engine_get_objective(const phovo_engine *e, int *objective);
/* Trust-region objective: solver options (kept under every objective, used by this one) and the per-pair solver records
 * of the LAST enqueue (n_pairs must be that enqueue's; PHOVO_E_UNSUPPORTED if it ran under another objective). */
int phovo_engine_set_trust_region_options(phovo_engine *e, const phovo_trust_region_options *opt);
int phovo_engine_get_trust_region_options(const phovo_engine *e, phovo_trust_region_options *opt);
int phovo_engine_fetch_trust_region_reports(phovo_engine *e, int n_pairs, phovo_trust_region_report *reports);
/* Affine-illumination objective: (alpha, beta) of every pair of the LAST enqueue (n_pairs must be that enqueue's;
 * PHOVO_E_NOT_READY before any enqueue, PHOVO_E_UNSUPPORTED if the last one ran under another objective). */
int phovo_engine_fetch_illumination(phovo_engine *e, int n_pairs, double *alpha_beta /* [n_pairs][2] */);
/* Photometric-geometric objective: options (kept under every objective, used by this one; every depth_weight must be finite
 * and > 0, else PHOVO_E_INVALID_ARGUMENT; a max_depth_residual <= 0 switches that level's gate off) and the per-pair records
 * of the LAST enqueue, with the call-order rules of phovo_engine_fetch_illumination. */
int phovo_engine_set_geometric_options(phovo_engine *e, const phovo_geometric_options *opt);
int phovo_engine_get_geometric_options(const phovo_engine *e, phovo_geometric_options *opt);
int phovo_engine_fetch_geometric_reports(phovo_engine *e, int n_pairs, phovo_geometric_report *reports);
/* Robust inverse-compositional objective: its option (kept under every objective, used by this one; scale_factor must be
 * finite and > 0, else PHOVO_E_INVALID_ARGUMENT) and the per-pair records of the LAST enqueue, with the call-order rules of
 * phovo_engine_fetch_geometric_reports. */
int phovo_engine_set_robust_options(phovo_engine *e, const phovo_robust_options *opt);
int phovo_engine_get_robust_options(const phovo_engine *e, phovo_robust_options *opt);
int phovo_engine_fetch_robust_reports(phovo_engine *e, int n_pairs, phovo_robust_report *reports);
/* Semi-dense inverse-compositional objective: its option (kept under every objective, used by this one; every
 * min_pixel_gradient must be finite and >= 0, else PHOVO_E_INVALID_ARGUMENT) and the per-pair records of the LAST enqueue,
 * with the call-order rules of phovo_engine_fetch_robust_reports. */
int phovo_engine_set_semidense_options(phovo_engine *e, const phovo_semidense_options *opt);
int phovo_engine_get_semidense_options(const phovo_engine *e, phovo_semidense_options *opt);
int phovo_engine_fetch_semidense_reports(phovo_engine *e, int n_pairs, phovo_semidense_report *reports);
/* Gaussian pose prior: the level scales (kept under every objective, used by phovo_engine_enqueue_align_prior; every
 * level_scale must be finite and >= 0, else PHOVO_E_INVALID_ARGUMENT; phovo_prior_options_default: 1 everywhere) and the
 * per-pair records of the LAST enqueue, with the call-order rules of phovo_engine_fetch_robust_reports
 * (PHOVO_E_UNSUPPORTED if the last enqueue carried no prior). */
int phovo_prior_options_default(phovo_prior_options *opt);
int phovo_engine_set_prior_options(phovo_engine *e, const phovo_prior_options *opt);
int phovo_engine_get_prior_options(const phovo_engine *e, phovo_prior_options *opt);
int phovo_engine_fetch_prior_reports(phovo_engine *e, int n_pairs, phovo_prior_report *reports);

/* Page-locks (and releases) a host buffer the caller will hand to the upload entry points repeatedly: uploads from
 * registered memory are direct DMA at the link rate instead of going through the runtime's bounce buffers.  Optional;
 * hipHostRegister / hipHostUnregister behind the C ABI for hosts that do not link the HIP runtime themselves, with the
 * library's own bookkeeping: registering a range that overlaps a registered one, and unregistering anything but the
 * start of a registered range, return PHOVO_E_INVALID_ARGUMENT (thread-safe). */
int phovo_host_register(void *ptr, size_t bytes);
int phovo_host_unregister(void *ptr);

/* (Re)allocates the frame pool: n_frames frames of width x height.  Uses the current config. */
int phovo_engine_reserve_frames(phovo_engine *e, int n_frames, int width, int height);
int phovo_engine_level_size(const phovo_engine *e, int level, int *width, int *height);
/* 1 if `level` is resident in the pool. */
int phovo_engine_level_is_stored(const phovo_engine *e, int level);

/* Copies one raw frame to the device and builds its pyramids there. depth may be NULL for a
 * pure target frame. */
int phovo_engine_upload_frame(phovo_engine *e, int frame, int roles,
                              const uint8_t *intensity, size_t intensity_stride,
                              const double *depth, size_t depth_stride);
/* Same with 16-bit depth (TUM / Kinect PNG) converted on the device as double(u16) * depth_scale
 * (apps/PhotoconsistencyVisualOdometry/PhotoconsistencyVisualOdometry.cpp:163,208,220). */
int phovo_engine_upload_frame_u16(phovo_engine *e, int frame, int roles,
                                  const uint8_t *intensity, size_t intensity_stride,
                                  const uint16_t *depth, size_t depth_stride, double depth_scale);
/* Batched forms: `count` consecutive pool slots starting at first_frame, frames `*_frame_stride` BYTES
 * apart in host memory (rows `*_stride` bytes apart).  One host->device copy and one producer launch per
 * pyramid level for up to 32 frames at a time, instead of a copy, six launches and a sync per frame. */
int phovo_engine_upload_frames(phovo_engine *e, int first_frame, int count, int roles,
                               const uint8_t *intensity, size_t intensity_stride, size_t intensity_frame_stride,
                               const double *depth, size_t depth_stride, size_t depth_frame_stride);
int phovo_engine_upload_frames_u16(phovo_engine *e, int first_frame, int count, int roles,
                                   const uint8_t *intensity, size_t intensity_stride, size_t intensity_frame_stride,
                                   const uint16_t *depth, size_t depth_stride, size_t depth_frame_stride,
                                   double depth_scale);
/* ---- frames that already live in device memory ---------------------------------------
 * A batch of images in DEVICE memory of the engine's device, with the caller's strides.  Formats:
 *   intensity  PHOVO_IMAGE_U8_GRAY            1 byte per pixel
 *              PHOVO_IMAGE_U8_RGB / _U8_BGR   3 interleaved bytes per pixel, reduced to gray on the device by
 *                                             (9797 R + 19234 G + 3737 B + 16384) >> 15 -- the project's one colour
 *                                             rule, the one apps/io/png_io.cpp applies to a colour PNG; integer
 *                                             arithmetic, so the device result equals read_gray8 on the same pixels
 *                                             exactly.  As that file says, the coefficients are RECALLED from OpenCV's
 *                                             cvtColor and could not be checked against it (OpenCV is absent here): this
 *                                             is NOT a claim of OpenCV parity.
 *   depth      PHOVO_IMAGE_F64                metres; depth_scale must be 1
 *              PHOVO_IMAGE_F32 / _F16 / _U16  depth = (double)value * depth_scale (one exact conversion, one fp64 multiply)
 * Rows are row_stride_bytes apart (>= width * bytes per pixel), frames frame_stride_bytes apart; for count > 1 a frame
 * must end before the next one starts (frame_stride_bytes >= (height - 1) * row_stride_bytes + width * bytes per
 * pixel); with count == 1 frame_stride_bytes is not looked at.  No alignment is required; rows and frames that start on
 * 16-byte boundaries (and a width of whole 16-byte groups) take the wide form of the packing kernel. */
#define PHOVO_IMAGE_U8_GRAY 0
#define PHOVO_IMAGE_U8_RGB  1
#define PHOVO_IMAGE_U8_BGR  2
#define PHOVO_IMAGE_F64     3
#define PHOVO_IMAGE_F32     4
#define PHOVO_IMAGE_F16     5
#define PHOVO_IMAGE_U16     6
typedef struct phovo_device_image {
  const void *data;          /* device pointer, on the engine's device */
  size_t row_stride_bytes;   /* >= width * bytes per pixel              */
  size_t frame_stride_bytes; /* distance between consecutive frames     */
  int    format;             /* PHOVO_IMAGE_*                            */
  int    reserved;           /* 0                                         */
} phovo_device_image;
/* phovo_engine_upload_frames[_u16] for frames in device memory: no host round trip.  The pool slots
 * first_frame .. first_frame + count - 1 end up holding exactly -- bit for bit, on every stored level, under every plane
 * storage, blur setting, role and objective -- the planes that the host upload of the same pixel values gives (for F32 /
 * F16 depth: of the fp64 values (double)value * depth_scale): one packing launch per kind and chunk of 32 frames writes
 * the engine's raw-frame staging buffers, and the same pyramid producers run on them.  depth may be NULL for pure target
 * frames (and is not read for them), except under the bi-objective.  `stream` is the hipStream_t on which the caller
 * produced the images (NULL: the default stream); it must belong to the engine's device.
 * Ordering -- there is no host synchronisation with the device work of this call (the first call, and a call that needs
 * larger staging buffers than any before, allocate them and wait for the engine's stream once):
 *   - the engine's stream waits, by event, for everything queued on `stream` before the call: the images need not be
 *     complete, only queued, when the call is made;
 *   - `stream` waits, by event, for the last kernel that reads the caller's memory: work queued on `stream` AFTER the
 *     call returns may overwrite or free the buffers.  The caller must NOT touch them from another stream or from the
 *     host, nor free them with hipFree from a thread that bypasses `stream`, until `stream` has passed that point
 *     (hipStreamSynchronize(stream) or an event recorded on it after the call);
 *   - the call waits on the host for every enqueue in flight before it queues anything, as the host uploads do;
 *   - phovo_engine_enqueue_align / align_pairs / evaluate_pairs, plane reads and writes, and later uploads are ordered
 *     behind the ingest on the device, as they are behind a host upload; the call itself returns before the pyramids exist.
 * Refusals, all before anything is queued and with the pool untouched (phovo_last_error names the argument):
 *   PHOVO_E_INVALID_ARGUMENT  NULL engine or intensity; a source role, or a bi-objective target, without depth; a frame
 *                             range outside the pool; empty roles; an unknown format, a depth format in `intensity` or an
 *                             intensity format in `depth`; row_stride_bytes smaller than a row; frames that overlap;
 *                             reserved != 0; depth_scale not finite, or not 1 with PHOVO_IMAGE_F64; a data pointer that
 *                             hipPointerGetAttributes does not report as plain device memory OF THE ENGINE'S DEVICE (a host
 *                             pointer, pinned or not, managed memory, another device's memory), or whose allocation
 *                             (hipMemGetAddressRange) is unknown or ends before the last frame does
 *   PHOVO_E_NOT_READY         no frame pool (phovo_engine_reserve_frames) */
int phovo_engine_upload_frames_device(phovo_engine *e, int first_frame, int count, int roles,
                                      const phovo_device_image *intensity,
                                      const phovo_device_image *depth /* NULL for pure targets */,
                                      double depth_scale, void *stream /* hipStream_t of the producer, NULL = default */);
/* What the last phovo_engine_upload_frames_device of this engine launched: staging chunks, and how many packing launches
 * took the wide (16-byte) and the scalar form. */
typedef struct phovo_ingest_record {
  int chunks;
  int wide_launches;
  int scalar_launches;
  int reserved;
} phovo_ingest_record;
int phovo_engine_last_ingest(const phovo_engine *e, phovo_ingest_record *out);
/* Single pair: Set*Frame (phovo_odometry_set_source_frame / _set_target_frame) for images in device memory:
 * phovo_engine_upload_frames_device with count 1 (same descriptors, same ordering on `stream`, same refusals -- checked before the pool is (re)allocated for a new size).  Like Set*Frame they drop the
 * evaluated-system state (phovo_odometry_get_pair_system is PHOVO_E_NOT_READY until the next Optimize()); the target's
 * depth is ignored (may be NULL) except under the bi-objective. */
int phovo_odometry_set_source_frame_device(phovo_odometry *o, const phovo_device_image *intensity,
                                           const phovo_device_image *depth, double depth_scale,
                                           int width, int height, void *stream);
int phovo_odometry_set_target_frame_device(phovo_odometry *o, const phovo_device_image *intensity,
                                           const phovo_device_image *depth, double depth_scale,
                                           int width, int height, void *stream);

/* Direct access to the planes of one level of one frame as fp64 (w*h doubles each, NULL = skip): lets a
 * caller supply pyramids built elsewhere (e.g. by OpenCV) or read back the device-built ones.  With a narrower
 * plane_storage, set rounds to the storage type and get returns the stored (rounded) values. */
int phovo_engine_set_level_planes(phovo_engine *e, int frame, int level,
                                  const double *intensity, const double *depth,
                                  const double *grad_x, const double *grad_y);
int phovo_engine_get_level_planes(const phovo_engine *e, int frame, int level,
                                  double *intensity, double *depth,
                                  double *grad_x, double *grad_y);
/* Bi-objective only (else PHOVO_E_UNSUPPORTED): the depth-gradient planes (w*h doubles each, NULL = skip) and the depth
 * gain of one level of one target frame.  phovo_engine_set_level_planes recomputes the gain of the level it writes and,
 * when it writes depth, the depth gradients with the max depth in force. */
int phovo_engine_get_level_depth_gradients(const phovo_engine *e, int frame, int level, double *grad_x, double *grad_y);
int phovo_engine_get_level_depth_gain(const phovo_engine *e, int frame, int level, double *gain);

/* Optimize() for n_pairs independent (source, target) frame pairs.
 *   init_states  n_pairs x 6 (SetInitialStateVector) or NULL for all-zero
 *   out_states   n_pairs x 6 optimal state vectors
 *   reports      n_pairs entries or NULL
 * Synchronous: returns when the results are in host memory. */
int phovo_engine_align_pairs(phovo_engine *e, int n_pairs,
                             const int *source_frames, const int *target_frames,
                             const double *init_states, double *out_states,
                             phovo_pair_report *reports);
/* Split form: enqueue without waiting, then wait, then fetch.  The argument arrays are copied before the call
 * returns.  (Levels that run in the wide form synchronise the stream every 8 iterations to look at the "done" words,
 * so for them the call returns when the level has finished.)  phovo_engine_synchronize waits for everything the engine
 * has in flight; fetch_results / results_device_ptr / last_align_ms / last_launches speak of the LAST enqueue. */
int phovo_engine_enqueue_align(phovo_engine *e, int n_pairs,
                               const int *source_frames, const int *target_frames,
                               const double *init_states);
/* phovo_engine_enqueue_align under a Gaussian pose prior per pair (phovo_prior_options above has the rule): the same
 * ticket, slot and ordering rules, and the prior travels with the enqueue -- two enqueues in flight keep their own.
 *   prior_states  n_pairs x 6: the prior poses, T_p = eigenPose(state)
 *   information   n_pairs x 36: Lambda row-major, twist order (nu, omega); the UPPER triangle is read
 * The level launches are PHOVO_LAUNCH_INVERSE_PRIOR / PHOVO_LAUNCH_INVERSE_ROBUST_PRIOR; phovo_engine_fetch_prior_reports
 * has e and e^T Lambda e of every pair.  The posterior information of a pair is the H that phovo_engine_evaluate_inverse_pairs
 * (or _robust_pairs) returns at its pose plus s_L Lambda.
 *   PHOVO_E_UNSUPPORTED       any objective but PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL and PHOVO_OBJECTIVE_INVERSE_ROBUST
 *   PHOVO_E_INVALID_ARGUMENT  NULL prior_states or information (with n_pairs > 0), a non-finite entry of either, a negative
 *                             diagonal entry of an information matrix; everything phovo_engine_enqueue_align refuses
 * A refused enqueue leaves the engine as it was. */
int phovo_engine_enqueue_align_prior(phovo_engine *e, int n_pairs,
                                     const int *source_frames, const int *target_frames,
                                     const double *init_states,
                                     const double *prior_states /* [n_pairs][6] */,
                                     const double *information /* [n_pairs][36] */);
int phovo_engine_synchronize(phovo_engine *e);
int phovo_engine_fetch_results(phovo_engine *e, int n_pairs, double *out_states,
                               phovo_pair_report *reports);
/* Device pointer to the n_pairs x 6 fp64 result of the last enqueue (for an RCCL gather). */
int phovo_engine_results_device_ptr(phovo_engine *e, void **states);

/* The Gauss-Newton system (phovo_pair_system) of n_pairs (source, target) frame pairs at the states [n_pairs][6] on one
 * level -- e.g. at the optimal states of an alignment, on the finest level it optimised, as information matrices for a
 * pose graph and costs to reject bad alignments.  Synchronous, like phovo_engine_align_pairs; ordered behind every
 * enqueue in flight, and it changes nothing that phovo_engine_fetch / fetch_results return.  Photometric objective with
 * nearest / scatter sampling, any plane storage, with or without Huber weights.
 *   PHOVO_E_UNSUPPORTED       bilinear sampling or the bi-objective
 *   PHOVO_E_INVALID_ARGUMENT  NULL pointers (with n_pairs > 0), n_pairs < 0, a frame index or level out of range
 *   PHOVO_E_NOT_READY         no intrinsics, the level is not stored (phovo_engine_level_is_stored), or a source frame
 *                             was not given its depth / a target frame its gradients (uploaded without that role)
 *                             on that level.  Roles are kept per frame AND level: an upload gives its roles on every
 *                             level, phovo_engine_set_level_planes on the level it writes (a depth plane: source, a
 *                             gradient plane: target).
 * n_pairs == 0 is OK.  Device memory: a workspace kept until the engine is destroyed -- per pair of a group 4 bytes of
 * owner map per pixel, 1 bit of ballots per pixel and 256 bytes of tile sums per 1024 pixels; large batches run in
 * groups whose owner maps take at most 256 MB (218 pairs at 640x480). */
int phovo_engine_evaluate_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt,
                                const double *states /* [n_pairs][6] */, int level, phovo_pair_system *out);

/* The same for the aligners that sample the target bilinearly (phovo_sampled_system): the photometric objective with
 * PHOVO_SAMPLING_BILINEAR (state_dim 6; either jacobian_corrected, any plane storage, with or without Huber weights) and
 * PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE (state_dim 8: pose, alpha, beta).  Synchronous; ordered behind every enqueue in
 * flight, and it changes nothing that phovo_engine_fetch / fetch_results / fetch_illumination return.
 *   PHOVO_E_UNSUPPORTED       the photometric objective with nearest / scatter sampling (phovo_engine_evaluate_pairs
 *                             serves it), the bi-objective, the trust-region objective
 *   PHOVO_E_INVALID_ARGUMENT  a state_dim that is not the mode's, NULL pointers (with n_pairs > 0), n_pairs < 0, a frame
 *                             index or level out of range
 *   PHOVO_E_NOT_READY         as phovo_engine_evaluate_pairs
 * n_pairs == 0 is OK.  Device memory: the evaluate workspace (shared with phovo_engine_evaluate_pairs, kept until the
 * engine is destroyed) -- per pair of a group 256 bytes (state_dim 6) or 512 bytes (state_dim 8) of tile sums per 1024
 * pixels; large batches run in groups whose tile sums take at most 64 MB. */
int phovo_engine_evaluate_sampled_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt,
                                        const double *states /* [n_pairs][state_dim] */, int state_dim, int level,
                                        phovo_sampled_system *out);

/* The system of PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC (phovo_geometric_system): the photometric and the depth block of
 * n_pairs pairs at the states [n_pairs][6] on one level, under the engine's phovo_geometric_options at that level.
 * Synchronous; ordered behind every enqueue in flight, and it changes nothing that phovo_engine_fetch / fetch_results /
 * fetch_geometric_reports return.
 *   PHOVO_E_UNSUPPORTED       any objective but PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC
 *   PHOVO_E_INVALID_ARGUMENT  as phovo_engine_evaluate_sampled_pairs
 *   PHOVO_E_NOT_READY         as phovo_engine_evaluate_sampled_pairs; also when a target frame lacks PHOVO_ROLE_SOURCE on
 *                             that level (its depth plane is a source upload's: the enqueue's rule)
 * n_pairs == 0 is OK.  Device memory: the evaluate workspace (shared with the other two evaluate calls, kept until the
 * engine is destroyed) -- per pair of a group 256 bytes of photometric and 256 bytes of depth tile sums per 1024 pixels;
 * large batches run in groups whose tile sums take at most 64 MB together (436 pairs at 640x480). */
int phovo_engine_evaluate_geometric_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt,
                                          const double *states /* [n_pairs][6] */, int level, phovo_geometric_system *out);

/* The system (phovo_pair_system) of the two objectives that are the reference's own other methods, at the states
 * [n_pairs][6] on one level; the call dispatches on the engine's objective.  Synchronous; ordered behind every enqueue in
 * flight, and it changes nothing that phovo_engine_fetch / fetch_results / fetch_trust_region_reports return.
 *   PHOVO_OBJECTIVE_TRUST_REGION  the rows the Levenberg-Marquardt aligner fills at that state: depth gate
 *       min_d < d < max_d, projection with true divisions, a pixel lands iff 0 <= u < W and 0 <= v < H on the real
 *       values, target W trunc(v) + trunc(u) owned by the largest source index landing there, r = I1(u, v) - I0 and the
 *       row from SampleLinear's taps with the exact warp Jacobian.  information = J^T J, gradient = J^T r, rows = owned
 *       targets, cost = r^T r: TWICE Ceres's cost (1/2 sum r^2) and twice phovo_trust_region_level.final_cost.
 *   PHOVO_OBJECTIVE_BIOBJECTIVE   the 2N-row system of the bi-objective aligner with the reference's row
 *       collisions: row m carries Jint(m) if m < N, m > 0 and pixel m contributes, else Jdep(m/2) if m is even and pixel
 *       m/2 contributes; its residual is that of the larger of owner[m] (m < N) and owner[m/2] (m even), a tie (m = 0)
 *       going to depth.  The gain and the depth-gradient planes are the ones resident for the target frame (made with the
 *       max depth in force at upload); the gate uses the depth range in force at the call.  information = J^T J and
 *       gradient = J^T r over all 2N rows, cost = r^T r over the whole 2N residual vector (entries whose Jacobian row is
 *       empty count), rows = contributing source pixels (what valid_pixels reports under this objective).
 * information is exactly symmetric (filled from the upper triangle).  flags: PHOVO_PAIR_RANK_DEFICIENT if rows < 6,
 * PHOVO_PAIR_NONFINITE if any sum is inf or NaN.  A pair's record is the same bit for bit whatever the batch, its position
 * in it, or any setting of the engine.
 *   PHOVO_E_UNSUPPORTED       the photometric objective (phovo_engine_evaluate_pairs or _evaluate_sampled_pairs serves
 *                             it), the affine-illumination objective (phovo_engine_evaluate_sampled_pairs), the
 *                             photometric-geometric objective (phovo_engine_evaluate_geometric_pairs)
 *   PHOVO_E_INVALID_ARGUMENT  NULL pointers (with n_pairs > 0), n_pairs < 0, a frame index or level out of range
 *   PHOVO_E_NOT_READY         as phovo_engine_evaluate_pairs
 * n_pairs == 0 is OK.  Device memory: the evaluate workspace (shared with the other evaluate calls, kept until the engine
 * is destroyed) -- per pair of a group 4 bytes of owner map per pixel, 1 bit of ballots per pixel and 256 bytes of tile
 * sums per 1024 pixels; large batches run in groups whose owner maps take at most 256 MB (218 pairs at 640x480). */
int phovo_engine_evaluate_objective_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt,
                                          const double *states /* [n_pairs][6] */, int level, phovo_pair_system *out);

/* The system (phovo_pair_system) of PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL in the TWIST basis, at the states [n_pairs][6]
 * on one level.  Synchronous; ordered behind every enqueue in flight, and it changes nothing that
 * phovo_engine_fetch / fetch_results return.
 *   pose      (R, t) = eigenPose(state): the state is the Euler state every other call takes and phovo_engine_fetch
 *             returns, and (R, t) is the matrix a level of the aligner starts from.
 *   rows      the aligner's (the objective's comment above): every source pixel in raster order with
 *             min_depth < D0 < max_depth (NaN fails), P' = R p + t, in bounds iff -0.5 < u < W - 0.5 and
 *             -0.5 < v < H - 0.5, I1(u, v) bilinear on four clamped taps, r = I1(u, v) - I0.
 *   J         (a, p x a) with a = (GX0 fx / pz, GY0 fy / pz, -(a_0 px + a_1 py) / pz) from the source frame's stored
 *             gradient planes; column order (nu_x, nu_y, nu_z, omega_x, omega_y, omega_z).
 *   record    information = sum J J^T (exactly symmetric, filled from the upper triangle), gradient = sum J r,
 *             cost = sum r^2 over the rows, rows = the count phovo_pair_report.valid_pixels uses; flags:
 *             PHOVO_PAIR_RANK_DEFICIENT if rows < 6, PHOVO_PAIR_NONFINITE if any sum is inf or NaN.  No weights: the
 *             objective has no Huber.
 * Perturbation: the system is that of T(xi) = T Exp(xi), where T = (R, t) takes points of the source camera into the
 * target camera: xi is a RIGHT-hand twist, expressed in the SOURCE camera's frame.  information^-1 * cost / (rows - 6)
 * is the covariance of that right-hand twist; a caller who perturbs on the left (Exp(xi') T) applies Ad_T on their
 * side (xi' = Ad_T xi).  No Euler-basis record of the other calls converts into this one without loss.
 * Relation to the aligner: the system the aligner solves in the FIRST iteration of a level is this system at the state the
 * level starts from, up to summation order; later iterations run on an (R, t) that no state holds exactly.
 * Sums are taken in an order that depends on the level size only: a pair's record is the same bit for bit whatever the
 * batch, its position in it, the group split, or any setting of the engine.
 *   PHOVO_E_UNSUPPORTED       any objective but PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL
 *   PHOVO_E_INVALID_ARGUMENT  as phovo_engine_evaluate_sampled_pairs (there is no state_dim)
 *   PHOVO_E_NOT_READY         as phovo_engine_evaluate_sampled_pairs; also when a SOURCE frame lacks PHOVO_ROLE_TARGET on
 *                             that level (its gradient planes are a target upload's: the enqueue's rule)
 * n_pairs == 0 is OK.  Device memory: the evaluate workspace (shared with the other evaluate calls, kept until the engine
 * is destroyed) -- per pair of a group 256 bytes of tile sums per 1024 pixels; large batches run in groups whose tile
 * sums take at most 64 MB (873 pairs at 640x480). */
int phovo_engine_evaluate_inverse_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt,
                                        const double *states /* [n_pairs][6] */, int level, phovo_pair_system *out);

/* The WEIGHTED system of PHOVO_OBJECTIVE_INVERSE_ROBUST in the TWIST basis, at the states [n_pairs][6] on one level
 * (DESIGN.md §23).  Synchronous; ordered behind every enqueue in flight, and it changes nothing that phovo_engine_fetch /
 * fetch_results / fetch_robust_reports return.
 *   pose, rows, r, J   exactly phovo_engine_evaluate_inverse_pairs': (R, t) = eigenPose(state), the aligner's rows,
 *             r = I1(u, v) - I0, J = (a, p x a), columns (nu_x, nu_y, nu_z, omega_x, omega_y, omega_z) of the right-hand
 *             perturbation T Exp(xi) in the source camera's frame.
 *   delta     deltas == NULL: delta = scale_factor * m, with m the objective's median rule (4096 bins,
 *             q = fabs(r) * 4096.0, bin q < 4096.0 ? (int)q : 4095, half = (n + 1) / 2, the same fp64 expression in the
 *             same order) on the residuals of THIS state and scale_factor from phovo_engine_set_robust_options; n = 0
 *             gives m = 0, delta = 0 and all sums zero.
 *             deltas != NULL: every entry finite and > 0 (else PHOVO_E_INVALID_ARGUMENT, before any launch); the weights
 *             use deltas[k], `delta` echoes it bit for bit, `median` is 0, and no histogram pass runs.  That is H(delta)
 *             for a caller's own threshold, and the system of any later iteration of the aligner at a state and the delta
 *             that phovo_robust_report names.
 *   sums      w = fabs(r) <= delta ? 1.0 : delta / fabs(r) (a true fp64 division); the record's fields below.  A NaN
 *             residual lands in the last bin and is counted in n; it is no outlier; it poisons the sums
 *             (PHOVO_PAIR_NONFINITE).
 * Relation to the aligner: its threshold lags one iteration and delta_1 = delta_0, the median at the entry pose, so the
 * system the aligner solves in the FIRST iteration of a level started at `state` is this record at `state` with
 * deltas == NULL, up to summation order.
 * Counts are integers and sums are taken in an order that depends on the level size only: a pair's record is the same bit
 * for bit whatever the batch, its position in it, the group split, or any setting of the engine.
 *   PHOVO_E_UNSUPPORTED       any objective but PHOVO_OBJECTIVE_INVERSE_ROBUST
 *   PHOVO_E_INVALID_ARGUMENT  as phovo_engine_evaluate_inverse_pairs; a deltas entry that is not finite and > 0
 *   PHOVO_E_NOT_READY         as phovo_engine_evaluate_inverse_pairs (source frames need PHOVO_ROLE_BOTH)
 * n_pairs == 0 is OK.  Device memory: the evaluate workspace -- per pair of a group 256 bytes of tile sums per 1024 pixels,
 * 16 KiB of histogram and 16 bytes for (m, delta); large batches run in groups that take at most 64 MB of these (720 pairs
 * at 640x480). */
int phovo_engine_evaluate_robust_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt,
                                       const double *states /* [n_pairs][6] */, const double *deltas /* [n_pairs] or NULL */,
                                       int level, phovo_robust_system *out);

/* Pipelining. Pairs are independent, and with data-dependent termination a batch ends with a few long pairs on an
 * otherwise idle chip.  The engine therefore keeps PHOVO_ENQUEUE_DEPTH enqueues in flight, each with its own stream, pair
 * buffers and pinned mirrors: phovo_engine_enqueue_align returns at once, and the kernels of enqueue k + 1 fill the CUs
 * that the tail of enqueue k leaves free.  Every enqueue gets a ticket (1, 2, ...; phovo_engine_last_ticket right after the
 * call); a ticket stays valid -- its results fetchable -- until PHOVO_ENQUEUE_DEPTH later enqueues have been issued.  The
 * slot an enqueue takes is waited for inside phovo_engine_enqueue_align, so a caller that never looks at tickets sees the
 * behaviour of a single stream, except that two consecutive enqueues may overlap on the device.  Uploads, plane writes
 * and configuration changes wait for every enqueue in flight before they touch device memory.
 *     for (k = 0; k < steps; k++) {
 *       phovo_engine_enqueue_align(e, n, src[k], tgt[k], NULL);  t[k] = phovo_engine_last_ticket(e);
 *       if (k > 0) phovo_engine_fetch(e, t[k - 1], n, states[k - 1], NULL);      // waits for enqueue k - 1 only
 *     }
 *     phovo_engine_fetch(e, t[steps - 1], n, states[steps - 1], NULL);
 * Results do not depend on what else is in flight (same kernels, same arithmetic per pair).
 * A refused enqueue (bad argument, a level that cannot run) takes no ticket and evicts nothing; one that fails later (an
 * allocation, a launch) leaves its slot empty, and every ticket-taking call refuses it.  An enqueue of zero pairs is an
 * enqueue (ticket, nothing to fetch, no device buffer).
 * Footprint: pair data (src, tgt, states, reports: 208 B per pair) and its pinned mirrors exist per slot; the large scratch
 * -- owner maps of levels above ~39 k pixels (4 B per pixel and pair: 10 GB for 8192 pairs on 640x480 level 0), ballots,
 * the wide form's workspace -- exists ONCE as long as the caller has one enqueue in flight at a time (it changes hands
 * between the slots) and twice only while two enqueues really overlap. */
#define PHOVO_ENQUEUE_DEPTH 2
int phovo_engine_last_ticket(const phovo_engine *e);                       /* 0 before the first enqueue */
int phovo_engine_wait(phovo_engine *e, int ticket);                        /* host wait for that enqueue alone */
int phovo_engine_fetch(phovo_engine *e, int ticket, int n_pairs, double *out_states, phovo_pair_report *reports);
int phovo_engine_device_states(phovo_engine *e, int ticket, void **states);    /* n_pairs x 6 fp64 in HBM */
int phovo_engine_align_ms(const phovo_engine *e, int ticket, double *total_ms, double level_ms[PHOVO_MAX_LEVELS]);

/* Device time (ms, HIP events on the enqueue's stream) of the last enqueue: first launch to last, and per level (0 for
 * levels that were not launched; a fused launch is reported at the coarsest level it covers). */
int phovo_engine_last_align_ms(const phovo_engine *e, double *total_ms,
                               double level_ms[PHOVO_MAX_LEVELS]);
/* What the last enqueue launched, in launch order: one record per kernel launch (the wide form: per level). */
enum { PHOVO_LAUNCH_PERSISTENT = 0,       /* gn_level_kernel: one level, one workgroup per pair at a time */
       PHOVO_LAUNCH_FUSED = 1,            /* gn_fused_kernel: levels level_first..level_last (coarse to fine) per pair */
       PHOVO_LAUNCH_SLIDE = 2,            /* gn_level_kernel_slide: owner ring in LDS */
       PHOVO_LAUNCH_SLIDE_FALLBACK = 3,   /* gn_level_kernel on the pairs the sliding-window launch handed over */
       PHOVO_LAUNCH_WIDE = 4,             /* k_wide_pass1 / k_wide_pass2 per iteration, many workgroups per pair */
       PHOVO_LAUNCH_BILINEAR = 5,         /* gn_level_kernel_bilinear (extension) */
       PHOVO_LAUNCH_BIOBJECTIVE = 6,      /* gn_level_kernel_biobjective (PHOVO_OBJECTIVE_BIOBJECTIVE) */
       PHOVO_LAUNCH_TRUST_REGION = 7,     /* gn_level_kernel_trust_region (PHOVO_OBJECTIVE_TRUST_REGION) */
       PHOVO_LAUNCH_AFFINE = 8,           /* gn_level_kernel_affine (PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE) */
       PHOVO_LAUNCH_GEOMETRIC = 9,        /* gn_level_kernel_geometric (PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) */
       PHOVO_LAUNCH_INVERSE = 10,         /* gn_level_kernel_inverse (PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL) */
       PHOVO_LAUNCH_INVERSE_ROBUST = 11,  /* gn_level_kernel_inverse_robust (PHOVO_OBJECTIVE_INVERSE_ROBUST) */
       PHOVO_LAUNCH_INVERSE_PRIOR = 12,   /* gn_level_kernel_inverse_prior (objective 5, phovo_engine_enqueue_align_prior) */
       PHOVO_LAUNCH_INVERSE_ROBUST_PRIOR = 13,    /* gn_level_kernel_inverse_prior, robust (objective 6, likewise) */
       PHOVO_LAUNCH_INVERSE_SEMIDENSE = 14 };     /* gn_level_kernel_inverse_semidense (PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) */
typedef struct phovo_launch_record {
  int level_first, level_last;            /* pyramid levels the launch covers (level_first >= level_last) */
  int kind;                               /* PHOVO_LAUNCH_* */
  int threads, lds_bytes, workgroups;     /* launch geometry (workgroups: grid size) */
} phovo_launch_record;
/* count receives the number of launches; up to `capacity` of them are written to out (may be NULL). */
int phovo_engine_last_launches(const phovo_engine *e, phovo_launch_record *out, int capacity, int *count);
/* Launch geometry chosen for `level` when it is launched alone: threads per workgroup and dynamic LDS bytes. */
int phovo_engine_level_launch_info(const phovo_engine *e, int level, int *threads, int *lds_bytes,
                                   int *owner_in_lds, int *source_in_lds);

#ifdef __cplusplus
}
#endif
#endif
