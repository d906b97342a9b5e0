// What the SAMPLED kernels share: the aligners that warp every source pixel to a real-valued target position and sample
// there bilinearly (gn_bilinear_kernel.hip, gn_affine_kernel.hip, gn_geometric_kernel.hip, and gn_inverse_kernel.hip and
// gn_inverse_robust_kernel.hip, which take the pair frame, the warp, the taps and bilerp and have a source-side row of
// their own) and the kernels that fill the
// same rows at a given state (k_eval_sampled, k_eval_geometric_depth, k_eval_inverse, through gn_evaluate_device.hpp).  An aligner and its
// "system at a given state" kernel promise exactly the same rows: the gates, the bounds test, the taps, the interpolation
// and the six pose columns stand here once, and a change to them is made here.
// TWIN, by measurement (comments at the places): gn_level_kernel_geometric has its own lines for pose_columns (both rows);
// the tap policies of gn_level_kernel_bilinear (one-sided clamps under the row mask) and of the fp64 form of
// gn_level_kernel_bilinear_dma (pair offsets, the 0 / 1 weight in the outer half-pixel band) stand in those kernels in
// place of clamped_taps.  A change to pose_columns or to clamped_taps goes into those too.
// Everything is __forceinline__ in an anonymous namespace, as in gn_device.hpp.  The warp and the columns have products
// feeding adds: they are for files compiled with default contraction only.  (Line numbers: ...Analytic.h.)
#pragma once

#include <hip/hip_runtime.h>

#include "gn_device.hpp"
#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

// ---- pair frame of the persistent aligners ---------------------------------------------------------------------------
// The fixed LDS of a level kernel (lds_fixed_bytes, with NBLOCKS blocks of sums per wave).  The helpers take it BY VALUE,
// and a kernel lambda copies it: by reference the compiler no longer sees that two rows of the sums lie 256 bytes apart
// (gn_level_kernel_geometric: 248 VGPRs instead of 246, 7 more instructions).
struct PairLds {
  double *cst;                            // [32] pose constants
  double *state;                          // [8]: the pose in the first 6
  double *red;                            // [NBLOCKS][NW][NRED]
  int *ctl;                               // [CTL_COUNT]
};
template <int NW, int NBLOCKS = 1>
__device__ __forceinline__ PairLds pair_lds(unsigned char *lds_raw)
{
  PairLds L;
  L.cst = reinterpret_cast<double *>(lds_raw);
  L.state = L.cst + 32;
  L.red = L.state + 8;
  L.ctl = reinterpret_cast<int *>(L.red + NBLOCKS * NW * NRED);
  return L;
}

// Head of the work-queue loop, as in gn_level_kernel (see there for the wait): the pair thread 0 drew last.
__device__ __forceinline__ int pair_drawn(const PairLds L)
{
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(L.ctl[CTL_PAIR]);
}

// Wave 0 loads the pair's state and writes its pose constants; lane 0 copies the state, runs more() (further state) and
// clears the control words.  Every thread reads them behind the closing barrier.
template <typename More>
__device__ __forceinline__ void pair_begin(const GNLevelArgs &A, int pair, int wave, int lane, const PairLds L, More more)
{
  if (wave == 0) {
    double st[6];
#pragma unroll
    for (int j = 0; j < 6; j++) st[j] = A.states[(size_t)pair * 6 + j];
    write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], L.cst, lane);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 6; j++) L.state[j] = st[j];
      more();
      L.ctl[CTL_DONE] = 0;
      L.ctl[CTL_FLAGS] = 0;
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void pair_begin(const GNLevelArgs &A, int pair, int wave, int lane, const PairLds L)
{
  pair_begin(A, pair, wave, lane, L, [] {});
}

// By thread 0 at the end of a pair: the pose back, more() (further state back), and the pair's report.
template <typename More>
__device__ __forceinline__ void pair_report(const GNLevelArgs &A, int pair, const PairLds L, int iterations, double gnorm,
                                            int valid, More more)
{
#pragma unroll
  for (int j = 0; j < 6; j++) A.states[(size_t)pair * 6 + j] = L.state[j];
  more();
  if (A.reports) {
    A.reports[pair].iterations[A.level] = iterations;
    A.reports[pair].gradient_norm = gnorm;
    A.reports[pair].valid_pixels[A.level] = valid;
    A.reports[pair].flags |= (uint32_t)L.ctl[CTL_FLAGS];
  }
}
__device__ __forceinline__ void pair_report(const GNLevelArgs &A, int pair, const PairLds L, int iterations, double gnorm,
                                            int valid)
{
  pair_report(A, pair, L, iterations, gnorm, valid, [] {});
}

// A lane's walk over the level in raster order, NW * WAVE pixels at a time: its first pixel k0 = (rd0, cd0), and the step.
struct LaneWalk {
  int k0;
  double cd0, rd0;
  RowColStep step;
};
template <int NW>
__device__ __forceinline__ LaneWalk lane_walk(int wave, int lane, int W)
{
  LaneWalk lw;
  lw.k0 = wave * WAVE + lane;
  const int r0 = lw.k0 / W, c0 = lw.k0 - r0 * W;
  const int step_r = (NW * WAVE) / W, step_c = (NW * WAVE) - step_r * W;
  lw.step = make_rowcol_step(step_r, step_c, W);
  lw.cd0 = (double)c0;
  lw.rd0 = (double)r0;
  return lw;
}

// ---- pose constants --------------------------------------------------------------------------------------------------
// The 21 constants of the block that the warp and the pose columns read, in scalar registers.
struct SampledPose {
  double cx, cyy, cz, r01, r02, r11, r12, t1, t2, t3, t4, t5, t6, t8, t14, t15, t16, t17, t24, cosy, siny;
  double t7, t9, t21;                     // -t6, -t8, -t5
};
__device__ __forceinline__ SampledPose sampled_pose(const double *s_cst)
{
  SampledPose P;
  const auto read = [&](int c) { return uniform_f64(s_cst[c]); };
  P.cx = read(C_X); P.cyy = read(C_Y); P.cz = read(C_Z);
  P.r01 = read(C_R01); P.r02 = read(C_R02);
  P.r11 = read(C_R11); P.r12 = read(C_R12);
  P.t1 = read(C_T1); P.t2 = read(C_T2); P.t3 = read(C_T3);
  P.t4 = read(C_T4); P.t5 = read(C_T5); P.t6 = read(C_T6);
  P.t8 = read(C_T8); P.t14 = read(C_T14); P.t15 = read(C_T15);
  P.t16 = read(C_T16); P.t17 = read(C_T17); P.t24 = read(C_T24);
  P.cosy = read(C_CY); P.siny = read(C_SY);
  P.t7 = -P.t6; P.t9 = -P.t8; P.t21 = -P.t5;
  return P;
}

// The pose as (R, t) in the same block, for a kernel that carries a rotation matrix instead of Euler angles
// (gn_inverse_kernel.hip): write_pose_constants leaves Rt in twelve of its slots -- rows (T15, R01, R02 | X),
// (T14, R11, R12 | Y), (-T3, T1, T2 | Z) -- and those twelve are all warp_project reads.  rt_constants_write puts a
// row-major R and t there (one lane calls it), sampled_pose_rt reads them back; the other members are 0 and nobody may
// hand such a pose to pose_columns.
__device__ __forceinline__ void rt_constants_write(double *s_cst, const double (&R)[9], const double (&t)[3])
{
  s_cst[C_T15] = R[0]; s_cst[C_R01] = R[1]; s_cst[C_R02] = R[2]; s_cst[C_X] = t[0];
  s_cst[C_T14] = R[3]; s_cst[C_R11] = R[4]; s_cst[C_R12] = R[5]; s_cst[C_Y] = t[1];
  s_cst[C_T3] = -R[6]; s_cst[C_T1] = R[7]; s_cst[C_T2] = R[8]; s_cst[C_Z] = t[2];
}
__device__ __forceinline__ void rt_constants_read(const double *s_cst, double (&R)[9], double (&t)[3])
{
  R[0] = s_cst[C_T15]; R[1] = s_cst[C_R01]; R[2] = s_cst[C_R02]; t[0] = s_cst[C_X];
  R[3] = s_cst[C_T14]; R[4] = s_cst[C_R11]; R[5] = s_cst[C_R12]; t[1] = s_cst[C_Y];
  R[6] = -s_cst[C_T3]; R[7] = s_cst[C_T1]; R[8] = s_cst[C_T2]; t[2] = s_cst[C_Z];
}
__device__ __forceinline__ SampledPose sampled_pose_rt(const double *s_cst)
{
  SampledPose P{};
  const auto read = [&](int c) { return uniform_f64(s_cst[c]); };
  P.cx = read(C_X); P.cyy = read(C_Y); P.cz = read(C_Z);
  P.r01 = read(C_R01); P.r02 = read(C_R02);
  P.r11 = read(C_R11); P.r12 = read(C_R12);
  P.t1 = read(C_T1); P.t2 = read(C_T2); P.t3 = read(C_T3);
  P.t14 = read(C_T14); P.t15 = read(C_T15);
  return P;
}

// The source-side row of the inverse-compositional objective (gn_inverse_kernel.hip and k_eval_inverse), twist order
// (nu, omega): with p = (px, py, pz) the unprojected source pixel and (gx, gy) the SOURCE frame's stored gradients,
//   a = (gx fx / pz, gy fy / pz, -(a_0 px + a_1 py) / pz),   J = (a, p x a).
// It depends on no pose: the aligner and its "system at a given state" kernel fill the same row from these six lines.
__device__ __forceinline__ void inverse_row(double (&J)[6], double gx, double gy, double px, double py, double pz, double fx,
                                            double fy)
{
  const double ipz = fast_rcp(pz);
  J[0] = (gx * fx) * ipz;
  J[1] = (gy * fy) * ipz;
  J[2] = -(J[0] * px + J[1] * py) * ipz;
  J[3] = py * J[2] - pz * J[1];                                           // p x a
  J[4] = pz * J[0] - px * J[2];
  J[5] = px * J[1] - py * J[0];
}

// ---- the warp --------------------------------------------------------------------------------------------------------
// Intrinsics, the depth gate and the bounds W - 0.5, H - 0.5, and the level size.
struct WarpFrame {
  double fx, fy, ox, oy, ifx, ify;
  double min_d, max_d, wlim, hlim;
  int n;
};
template <typename Args>
__device__ __forceinline__ WarpFrame warp_frame(const Args &A)
{
  return {A.fx, A.fy, A.ox, A.oy, A.ifx, A.ify, A.min_depth, A.max_depth, (double)A.w - 0.5, (double)A.h - 0.5, A.n};
}

struct WarpTarget { double tc, tr; };     // the real-valued target column and row
// Source pixel k = (rd, cd) of depth pz through the pose: the row's geometry w.px, py, pz, Zr, t25 and the row mask w.m.
// Depth gate (:280), and in bounds iff the NEAREST pixel is inside -- the same region as the reference's round() test
// (:297-303), so a zero-motion start never sits on the boundary (NaN fails the comparisons).  One ballot per comparison,
// ANDed on the scalar unit.
template <typename Warped>
__device__ __forceinline__ WarpTarget warp_project(Warped &w, int k, double cd, double rd, double pz, const SampledPose &P,
                                                   const WarpFrame &F)
{
  const double px = (cd - F.ox) * pz * F.ifx;                             // :282
  const double py = (rd - F.oy) * pz * F.ify;                             // :283
  const double X = ((P.t15 * px + P.r01 * py) + P.r02 * pz) + P.cx;       // :291
  const double Y = ((P.t14 * px + P.r11 * py) + P.r12 * pz) + P.cyy;
  const double Zr = py * P.t1 + pz * P.t2 - px * P.t3;
  const double t25 = fast_rcp(P.cz + Zr);                                 // :294 and :313 are the same quantity
  const double tc = (X * F.fx) * t25 + F.ox;                              // :295
  const double tr = (Y * F.fy) * t25 + F.oy;                              // :296
  w.m = __builtin_amdgcn_ballot_w64(k < F.n) & __builtin_amdgcn_ballot_w64(F.min_d < pz) &
        __builtin_amdgcn_ballot_w64(pz < F.max_d) & __builtin_amdgcn_ballot_w64(tc > -0.5) &
        __builtin_amdgcn_ballot_w64(tc < F.wlim) & __builtin_amdgcn_ballot_w64(tr > -0.5) &
        __builtin_amdgcn_ballot_w64(tr < F.hlim);
  w.px = px; w.py = py; w.pz = pz; w.Zr = Zr; w.t25 = t25;
  return {tc, tr};
}

// The cell of the target position: w.ax, w.ay the bilinear weights, (ir, ic) the row and column of tap p00.
// (Lanes outside w.m: whatever the conversions give.)
struct WarpCell { int ic, ir; };
template <typename Warped>
__device__ __forceinline__ WarpCell warp_cell(Warped &w, const WarpTarget &t)
{
  const double fc = floor(t.tc), fr = floor(t.tr);
  w.ax = t.tc - fc;
  w.ay = t.tr - fr;
  return {(int)fc, (int)fr};
}

// Clamp-to-edge taps p00, p01, p10, p11 as indices into a plane (in the outer half-pixel band both taps of a row / a column
// are the edge pixel): every index lies in [0, n), also in lanes outside the row mask, whose taps nobody uses.
__device__ __forceinline__ void clamped_taps(int (&idx)[4], const WarpCell &c, int W, int H)
{
  const int r0w = __mul24(min(max(c.ir, 0), H - 1), W), r1w = __mul24(min(max(c.ir + 1, 0), H - 1), W);
  const int c0i = min(max(c.ic, 0), W - 1), c1i = min(max(c.ic + 1, 0), W - 1);
  idx[0] = r0w + c0i; idx[1] = r0w + c1i; idx[2] = r1w + c0i; idx[3] = r1w + c1i;
}

// ---- the row ---------------------------------------------------------------------------------------------------------
// The bilinear interpolant at weights (ax, ay) of the taps p00, p01 (upper row), p10, p11.
__device__ __forceinline__ double bilerp(double ax, double ay, double p00, double p01, double p10, double p11)
{
  return (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11);
}

// The six pose columns J = gx dU/dp + gy dV/dp - minus_z dZ'/dp of the row whose geometry is w.  CORRECTED selects the true
// warp Jacobian (temp11 = temp15, i.e. without the reference's `+x` transcription slip, :253) instead of the reference's.
// dZ'/dp is (0, 0, 1, 0, Cm, Dm), and since columns 4 and 5 take Cm and Dm times column 2, minus_z goes in there once (the
// depth row of the photometric-geometric objective; 0 for an intensity row, whose subtraction the compiler drops: exact).
template <bool CORRECTED, typename Warped>
__device__ __forceinline__ void pose_columns(double (&J)[6], double gx, double gy, const Warped &w, const SampledPose &P,
                                             double fx, double fy, double minus_z = 0.0)
{
  const double px = w.px, py = w.py, pz = w.pz, Zr = w.Zr, t25 = w.t25;
  const double base = pz * P.t4 + py * P.t5 + px * P.t15;                 // (pz*temp4+py*temp5+px*temp15) = X - x
  const double Au = CORRECTED ? base + P.cx : base + px * P.cx;           // reference: px*(temp15 + x)  (:253)
  const double Bv = py * P.t6 + pz * P.t9 + px * P.t14 + P.cyy;
  const double Cm = -py * P.t16 - pz * P.t17 - px * P.t24;                // dZ'/dpitch
  const double Dm = py * P.t2 - pz * P.t1;                                // dZ'/droll
  J[0] = (gx * fx) * t25;
  J[1] = (gy * fy) * t25;
  J[2] = -(J[0] * Au + J[1] * Bv) * t25 - minus_z;
  J[3] = J[0] * (P.cyy - Bv) + J[1] * base;
  J[4] = (J[0] * P.cosy + J[1] * P.siny) * Zr + Cm * J[2];
  J[5] = J[0] * (py * P.t4 + pz * P.t21) + J[1] * (pz * P.t7 + py * P.t9) + Dm * J[2];
}

}  // namespace

}  // namespace phovo_hip
