// Device-side building blocks shared by the Gauss-Newton kernels (gn_kernels.hip, gn_wide_kernels.hip):
// pose constants, wave / workgroup reductions, the 6x6 solve, typed plane loads.  Everything is
// __forceinline__ in an anonymous namespace: each translation unit gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

constexpr int WAVE = 64;
constexpr size_t LDS_LIMIT = 160 * 1024;   // MI355X: 160 KiB per CU, one workgroup may take all of it
constexpr int NRED = 32;     // padded for the butterfly
constexpr int RED_VALID = 27;   // slot behind the 21 + 6 sums: the number of Jacobian rows filled (lane 0 of every wave puts
                                // its wave's count there as a double -- exact -- and the reduction adds them up for free)

// Indices into the pose-constant block in LDS.
enum {
  C_X = 0, C_Y, C_Z, C_R01, C_R02, C_R11, C_R12,
  C_T1, C_T2, C_T3, C_T4, C_T5, C_T6, C_T8, C_T11, C_T14, C_T15,
  C_T16, C_T17, C_T24, C_CY, C_SY, C_COUNT
};

// Control words in LDS.
enum { CTL_DONE = 0, CTL_FLAGS = 1, CTL_PAIR = 2, CTL_OOW = 3, CTL_COUNT = 4 };      // CTL_OOW: sliding-window kernel only

// LDS every level kernel needs beside its maps: pose constants [32], state [8], one row of NRED wave sums per wave, control words
__host__ __device__ constexpr size_t lds_fixed_bytes(int threads)
{
  return sizeof(double) * (32 + 8 + (size_t)(threads / WAVE) * NRED) + sizeof(int) * CTL_COUNT;
}

// A workgroup barrier behind which every LDS access issued in front of it has completed.
__device__ __forceinline__ void lds_barrier()
{
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

__device__ __forceinline__ double uniform_f64(double v)
{
  // The value is identical in every lane: move it to scalar registers so that the per-pixel
  // math reads it as an SGPR operand instead of burning two VGPRs per constant.
  int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// Data-parallel-primitive moves (v_mov_b32 with a DPP modifier): a lane reads another lane of its own 16-lane row straight
// from the register file -- no LDS crossbar (ds_bpermute, what __shfl compiles to) and no round trip to wait for.
// Controls: quad_perm is its four 2-bit selectors, row_ror:n is 0x120 + n and means "lane l reads lane (l - n) mod 16 of
// its row".  The bank mask enables the destination's banks of four lanes (bit b: lanes 4b .. 4b+3 of every row); a lane it
// leaves out keeps `old`.  Every lane of the wave must be active where these are used.
constexpr int DPP_QUAD_XOR1 = 0xB1;       // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;       // quad_perm:[2,3,0,1]
constexpr int DPP_QUAD_BCAST1 = 0x55;     // quad_perm:[1,1,1,1]
constexpr int DPP_QUAD_BCAST2 = 0xAA;     // quad_perm:[2,2,2,2]
constexpr int DPP_ROW_ROR = 0x120;
template <int CTRL, int BANKS = 0xf>
__device__ __forceinline__ double dpp_f64(double old, double src)
{
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, BANKS, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, BANKS, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double src) { return dpp_f64<CTRL>(src, src); }

// sin / cos of the three Euler angles: valid in lane 0 on return (the whole wave executes this with a wave-uniform state).
__device__ __forceinline__ void pose_sincos_lane0(double yaw, double pitch, double roll, int lane, double &sy, double &cy,
                                                  double &sp, double &cp, double &sr, double &cr)
{
  // Lanes 0, 1, 2 take yaw, pitch, roll: ONE sincos issue instead of three dependent ones; the six
  // results are then broadcast (the whole wave executes this with a wave-uniform state).
  const double ang = (lane == 1) ? pitch : ((lane == 2) ? roll : yaw);
  double sn, cs;
  // Euler angles of a frame-to-frame motion are small: up to pi/4 the two minimax polynomials of fdlibm's __kernel_sin /
  // __kernel_cos (errors below one ulp, as the library's) need no argument reduction; anything larger takes the device
  // library's sincos (wave-uniform branch: lanes 3.. carry yaw).  The library call alone cost 4.7 k cycles per iteration
  // for a reason that has nothing to do with arithmetic: its polynomial coefficients are VGPR immediates that the
  // compiler hoists to the top of the kernel, cannot keep under the 128-register cap and SPILLS -- nine dependent
  // scratch reloads, each a full trip to memory behind an s_waitcnt vmcnt(0), in the middle of wave 0's serial section
  // (and nine more in every pair's prologue).  Here the coefficients are scalar operands (opaque to the hoisting).
  const bool small_angles = __builtin_amdgcn_ballot_w64(!(fabs(ang) <= 0.78539816339744828)) == 0;
  if (small_angles) {
    auto k = [](double v) { asm volatile("" : "+s"(v)); return v; };       // a coefficient as an SGPR pair
    const double z = ang * ang;
    double ps = fma(z, k(1.58969099521155010221e-10), k(-2.50507602534068634195e-08));
    double pc = fma(z, k(-1.13596475577881948265e-11), k(2.08757232129817482790e-09));
    ps = fma(z, ps, k(2.75573137070700676789e-06));
    pc = fma(z, pc, k(-2.75573143513906633035e-07));
    ps = fma(z, ps, k(-1.98412698298579493134e-04));
    pc = fma(z, pc, k(2.48015872894767294178e-05));
    ps = fma(z, ps, k(8.33333333332248946124e-03));
    pc = fma(z, pc, k(-1.38888888888741095749e-03));
    ps = fma(z, ps, k(-1.66666666666666324348e-01));
    pc = fma(z, pc, k(4.16666666666666019037e-02));
    sn = fma(ang * z, ps, ang);                         // x + x^3 (S1 + z (S2 + ...)): 0.63 ulp at worst
    // cos = 1 - z/2 + z^2 (C1 + z (C2 + ...)), summed as fdlibm does: from 0.3 upwards a quarter of |x| (truncated to
    // its high word, so that 1 - qx and z/2 - qx are exact) is taken out of both big terms first: 0.77 ulp at worst
    // (1.2 ulp summed naively)
    const double ax = fabs(ang);
    const double q4 = __hiloint2double(__double2hiint(ax) - 0x00200000, 0);
    const double qx = ax < 0.3 ? 0.0 : (ax > 0.78125 ? 0.28125 : q4);
    cs = (1.0 - qx) - fma(-z, z * pc, 0.5 * z - qx);
  } else {
    sincos(ang, &sn, &cs);
  }
  // Only lane 0 goes on: it has yaw's pair itself and takes pitch's and roll's from lanes 1 and 2 of its own quad with
  // two DPP moves per value (quad_perm), not through the LDS crossbar (twelve ds_bpermute and their round trip before).
  sy = sn; cy = cs;
  sp = dpp_f64<DPP_QUAD_BCAST1>(sn); cp = dpp_f64<DPP_QUAD_BCAST1>(cs);
  sr = dpp_f64<DPP_QUAD_BCAST2>(sn); cr = dpp_f64<DPP_QUAD_BCAST2>(cs);
}

// Pose constants from the state: Rt (:219-241) and temp1..temp24 (:243-266), written with the
// reference's association.  temp7 = -temp6, temp9 = -temp8, temp21 = -temp5, temp22 = temp2,
// temp23 = temp1 hold exactly in IEEE arithmetic and are not stored; Rt(0,0) = temp15,
// Rt(1,0) = temp14, Rt(2,0) = -temp3, Rt(2,1) = temp1, Rt(2,2) = temp2 likewise.  temp10, temp12, temp13 are
// temp1, temp2, temp3 times cos(yaw) and temp18, temp19, temp20 the same times sin(yaw): the kernel applies
// those two factors to the sum instead (the sampled kernels' row, gn_sampled_device.hpp; in analytic_row below they are the
// pitch axis), so only cos(yaw) and sin(yaw) are stored.
__device__ __forceinline__ void write_pose_constants(double x, double y, double z, double yaw, double pitch,
                                                     double roll, double *cst, int lane)
{
  double sy, cy, sp, cp, sr, cr;
  pose_sincos_lane0(yaw, pitch, roll, lane, sy, cy, sp, cp, sr, cr);
  if (lane != 0) return;
  cst[C_X] = x; cst[C_Y] = y; cst[C_Z] = z;
  cst[C_R01] = cy * sp * sr - sy * cr;
  cst[C_R02] = cy * sp * cr + sy * sr;
  cst[C_R11] = sy * sp * sr + cy * cr;
  cst[C_R12] = sy * sp * cr - cy * sr;
  cst[C_T1] = cp * sr;
  cst[C_T2] = cp * cr;
  cst[C_T3] = sp;
  cst[C_T4] = sr * sy + sp * cr * cy;
  cst[C_T5] = sp * sr * cy - cr * sy;
  cst[C_T6] = sp * sr * sy + cr * cy;
  cst[C_T8] = sr * cy - sp * cr * sy;
  cst[C_T11] = cp * cy + x;          // the reference's bug, kept (:253)
  cst[C_T14] = cp * sy;
  cst[C_T15] = cp * cy;
  cst[C_T16] = sp * sr;
  cst[C_T17] = sp * cr;
  cst[C_T24] = cp;
  cst[C_CY] = cy;
  cst[C_SY] = sy;
}

// The same block as the level kernels (gn_kernels.hip, level_body) keep it: what their two passes CONSUME, in the order
// they read it, so that every read is one half of a 16-byte pair at a wave-uniform address.  Pass 1 takes slots
// P_FR00 .. P_T3: the rotation entries as scalars, the translation and the unprojection offsets P_XF .. P_Z as
// lane-uniform values in vector registers (a value read from LDS is in a vector register already: handing it to the
// scalar file and back cost two v_readfirstlane_b32 and a v_mov_b64 per constant, in every wave and iteration); pass 2,
// at the register cap, takes P_OXI .. P_Y, all but three of them as scalars, and keeps pass 1's P_T1 .. P_T3.
// The focal products are Rt's two projected rows and the translation times fx / fy: each the one product of
// the same two operands that every wave used to form for itself, now formed once, by the lane that writes the block.
// P_OXI, P_OYI belong to the level, not to the pose: written by the level's prologue (level_body), never here.
enum {
  P_FR00 = 0, P_FR01, P_FR02, P_FR10, P_FR11, P_FR12, P_XF, P_YF,
  P_OXI, P_OYI, P_Z, P_T1, P_T2, P_T3,
  P_T4, P_T5, P_T6, P_T8, P_T11, P_T14, P_T15, P_CY, P_SY, P_X, P_Y, P_COUNT
};
static_assert(P_COUNT <= 32 && P_OXI % 2 == 0, "the block has 32 slots; pass 2's first read starts a 16-byte pair");

__device__ __forceinline__ void write_pass_constants(double x, double y, double z, double yaw, double pitch, double roll,
                                                     double fx, double fy, double *cst, int lane)
{
  double sy, cy, sp, cp, sr, cr;
  pose_sincos_lane0(yaw, pitch, roll, lane, sy, cy, sp, cp, sr, cr);
  if (lane != 0) return;
  // (the factors of the focal products are rounded values of their own, as they were when they came out of the block:
  // opaque, so that no product is folded into the expression in front of it)
  auto rounded = [](double v) { asm volatile("" : "+v"(v)); return v; };
  const double r01 = rounded(cy * sp * sr - sy * cr), r02 = rounded(cy * sp * cr + sy * sr);
  const double r11 = rounded(sy * sp * sr + cy * cr), r12 = rounded(sy * sp * cr - cy * sr);
  const double t14 = rounded(cp * sy), t15 = rounded(cp * cy);
  cst[P_FR00] = t15 * fx; cst[P_FR01] = r01 * fx; cst[P_FR02] = r02 * fx;
  cst[P_FR10] = t14 * fy; cst[P_FR11] = r11 * fy; cst[P_FR12] = r12 * fy;
  cst[P_XF] = x * fx; cst[P_YF] = y * fy;
  cst[P_Z] = z;
  cst[P_T1] = cp * sr;
  cst[P_T2] = cp * cr;
  cst[P_T3] = sp;
  cst[P_T4] = sr * sy + sp * cr * cy;
  cst[P_T5] = sp * sr * cy - cr * sy;
  cst[P_T6] = sp * sr * sy + cr * cy;
  cst[P_T8] = sr * cy - sp * cr * sy;
  cst[P_T11] = cp * cy + x;          // the reference's bug, kept (:253)
  cst[P_T14] = t14;
  cst[P_T15] = t15;                  // Rt's first column (t15, t14, -t3) is the roll axis of the row (analytic_row)
  cst[P_CY] = cy;
  cst[P_SY] = sy;
  cst[P_X] = x; cst[P_Y] = y;
}

// One butterfly stage of the transposed wave reduction at a distance inside a 16-lane row: N values in, N/2 out.  For the
// pair (v[i], v[i + N/2]) a lane with bit DIST of its index clear keeps v[i] and receives its partner's v[i] (the partner
// is lane ^ DIST), a lane with the bit set keeps v[i + N/2] and receives its partner's: v[i] = keep + received.
// Nothing travels through the LDS crossbar (the four stages were four dependent ds_bpermute round trips, which the last
// wave of a workgroup pays in the open in front of the barrier):
//   DIST 8, 4  the bit splits a row into whole banks of four lanes, so two DPP moves per dword under bank masks build
//              A = { own v[i] | partner's v[i + N/2] } and B = { partner's v[i] | own v[i + N/2] } (clear | set) without a
//              select, and A + B is keep + received (as in reduce_stage_swap below).  xor 8 is row_ror:8 for every lane;
//              xor 4 is row_ror:12 (reads lane + 4) for the clear banks and row_ror:4 (reads lane - 4) for the set ones.
//   DIST 2, 1  inside a quad: select what to send, one quad_perm move per dword.
// The stage is issued in groups of G exchanges with a scheduling fence between groups: left alone, the scheduler hoists
// all N/2 exchanges' moves in front of the adds and the live range grows by 4 VGPRs per exchange
// (179 VGPRs and spills under the 128-register budget of a 1024-thread workgroup).
// (In the lanes with the bit set A + B is received + keep, in the others keep + received: the same sum bit for bit unless
// both are NaNs of different payloads; reduce_stage_swap has the same property.)
template <int N, int G, int DIST>
__device__ __forceinline__ void reduce_stage(double (&v)[NRED], int lane)
{
  static_assert(DIST == 8 || DIST == 4 || DIST == 2 || DIST == 1, "a distance inside a 16-lane row");
#pragma unroll
  for (int base = 0; base < N / 2; base += G) {
#pragma unroll
    for (int i = base; i < base + G && i < N / 2; i++) {
      if constexpr (DIST >= 4) {
        constexpr int SET = DIST == 8 ? 0xc : 0xa, CLEAR = 0xf ^ SET;       // banks of the lanes with the bit set / clear
        constexpr int FROM_BELOW = DPP_ROW_ROR + DIST, FROM_ABOVE = DPP_ROW_ROR + 16 - DIST;
        const double a = dpp_f64<FROM_BELOW, SET>(v[i], v[i + N / 2]);
        const double b = dpp_f64<FROM_ABOVE, CLEAR>(v[i + N / 2], v[i]);
        v[i] = a + b;
      } else {
        const bool up = (lane & DIST) != 0;
        const double send = up ? v[i] : v[i + N / 2];
        const double keep = up ? v[i + N / 2] : v[i];
        v[i] = keep + dpp_f64<DIST == 2 ? DPP_QUAD_XOR2 : DPP_QUAD_XOR1>(send);
      }
    }
    if (N / 2 > G) __builtin_amdgcn_sched_barrier(0);
  }
}

// The two widest butterfly stages without selects or LDS-crossbar traffic: gfx950's
// v_permlane32_swap / v_permlane16_swap exchange the upper half (odd 16-lane rows) of one register with
// the lower half (even rows) of another, so for the pair (v[i], v[i+N/2]) one swap per dword leaves
//   newA = { own v[i] in the low lanes,  partner's v[i+N/2] in the high lanes }
//   newB = { partner's v[i] in the low lanes,  own v[i+N/2] in the high lanes }
// and newA + newB is exactly "keep + received" of reduce_stage with the same lane -> index map.
template <int N, bool ROW16>
__device__ __forceinline__ void reduce_stage_swap(double (&v)[NRED])
{
#pragma unroll
  for (int i = 0; i < N / 2; i++) {
    const unsigned alo = (unsigned)__double2loint(v[i]), ahi = (unsigned)__double2hiint(v[i]);
    const unsigned blo = (unsigned)__double2loint(v[i + N / 2]), bhi = (unsigned)__double2hiint(v[i + N / 2]);
    const auto lo = ROW16 ? __builtin_amdgcn_permlane16_swap(alo, blo, false, false)
                          : __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    const auto hi = ROW16 ? __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false)
                          : __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    v[i] = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
  }
}

// 6x6 solve of the normal equations H x = g by an unpivoted LDL^T factorisation: H = J^T J is
// symmetric positive semi-definite, for which LDL^T is backward stable, needs 6 reciprocals instead of
// the 21 divisions + 15 row swaps of pivoted elimination and only the 21 upper-triangular sums.
// (The reference forms H^-1 with Eigen's PartialPivLU, ...Analytic.h:540; both are accurate to
// cond(H)*eps, far inside the 1e-5 pose bar -- tests/test_gpu_parity.py holds 1e-9.  tests/test_gpu_device_arith.py holds
// this solver and the two below to |x - x_exact| <= c cond2(H) 2^-53 |x_exact| directly)
// h is the upper triangle, row-major: h[idx(i,j)], i <= j.  Fully unrolled: every index is a
// compile-time constant, nothing goes to scratch.
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

__device__ __forceinline__ void solve6_ldlt(const double (&h)[21], const double (&g)[6], double (&x)[6])
{
  double L[6][6];       // strictly lower part used
  double Ld[6][6];      // L[i][k] * d[k]
  double inv[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double dj = h[tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) dj = fma(-L[j][k], Ld[j][k], dj);
    inv[j] = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double t = h[tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; k++) t = fma(-L[i][k], Ld[j][k], t);
      Ld[i][j] = t;
      L[i][j] = t * inv[j];
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double t = g[i];
#pragma unroll
    for (int k = 0; k < i; k++) t = fma(-L[i][k], y[k], t);
    y[i] = t;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double t = y[i] * inv[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) t = fma(-L[k][i], x[k], t);
    x[i] = t;
  }
}

// (The trust-region kernel's; gn_trust_region_kernel.hip compiles it, as everything it includes, with fp contraction off.)
__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// 6x6 Cholesky factorisation in place (a: upper triangle, row-major, becomes L^T) and solve of A y = b.  False if a pivot
// is not positive (or not finite).
__device__ __forceinline__ bool solve6_cholesky(double (&a)[21], const double (&b)[6], double (&y)[6])
{
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = a[tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) d = fma(-a[tri(k, j)], a[tri(k, j)], d);
    ok = ok && d > 0.0 && finite_f64(d);
    const double ljj = sqrt(d);
    a[tri(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double t = a[tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; k++) t = fma(-a[tri(k, i)], a[tri(k, j)], t);
      a[tri(j, i)] = t / ljj;                   // L[i][j]
    }
  }
  double z[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double t = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) t = fma(-a[tri(k, i)], z[k], t);
    z[i] = t / a[tri(i, i)];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double t = z[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) t = fma(-a[tri(i, k)], y[k], t);
    y[i] = t / a[tri(i, i)];
  }
  return ok;
}

// The affine-illumination kernel's parameters (gn_affine_kernel.hip): the pose and (alpha, beta)
constexpr int NP = 8;
// The 6 x 6 solve above (unpivoted LDL^T, every index a compile-time constant) extended to 8 x 8.
__device__ __forceinline__ constexpr int tri8(int i, int j) { return i * NP - (i * (i - 1)) / 2 + (j - i); }

__device__ __forceinline__ void solve8_ldlt(const double (&h)[36], const double (&g)[NP], double (&x)[NP])
{
  double L[NP][NP];     // strictly lower part used
  double Ld[NP][NP];    // L[i][k] * d[k]
  double inv[NP];
#pragma unroll
  for (int j = 0; j < NP; j++) {
    double dj = h[tri8(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) dj = fma(-L[j][k], Ld[j][k], dj);
    inv[j] = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < NP; i++) {
      double t = h[tri8(j, i)];
#pragma unroll
      for (int k = 0; k < j; k++) t = fma(-L[i][k], Ld[j][k], t);
      Ld[i][j] = t;
      L[i][j] = t * inv[j];
    }
  }
  double y[NP];
#pragma unroll
  for (int i = 0; i < NP; i++) {
    double t = g[i];
#pragma unroll
    for (int k = 0; k < i; k++) t = fma(-L[i][k], y[k], t);
    y[i] = t;
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; i--) {
    double t = y[i] * inv[i];
#pragma unroll
    for (int k = i + 1; k < NP; k++) t = fma(-L[k][i], x[k], t);
    x[i] = t;
  }
}

// Plane loads go through buffer descriptors: the four planes of a chunk share ONE 32-bit byte offset
// (8*k) in a VGPR while the bases sit in SGPRs, and a read past the plane returns 0 instead of needing
// a branch (raw buffer, num_records = plane bytes).  Flat loads cost a 64-bit VGPR address per plane.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const unsigned char *p, int n)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(p), 0, n * (int)sizeof(T), 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t frame_rsrc(const unsigned char *frame, size_t frame_bytes)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(frame), 0, (int)frame_bytes, 0x00020000);
}
// Element `idx` of a plane stored as T, widened to fp64 exactly, subnormals included (all arithmetic stays fp64; narrower
// storage is the opt-in extension of include/phovo_hip.h, PHOVO_STORAGE_*).  idx = -1 or past the DESCRIPTOR reads 0.
// soff: a wave-uniform byte offset (the instruction's scalar offset; it takes part in the range check: a read is served
// iff soff + idx * sizeof(T) + sizeof(T) <= num_records, tests/test_gpu_device_arith.py): one descriptor
// per FRAME (frame_rsrc) serves every plane of it -- base = the frame, soff = the plane's offset in it.  Four SGPRs per
// frame plus one per plane instead of four per plane: the level kernels run out of scalar registers, and every spilled
// one costs a v_readlane per use in the pixel loops.
// With a frame descriptor "past the plane" is therefore NOT 0 while the address is still inside the frame: it is the
// element of the plane that lies there (behind the frame it is 0 again, so nothing outside the frame is ever read).
// Every read of that kind is a chunk-ahead prefetch or the tail of the last, partial chunk, whose lanes the in-image
// mask drops; an owner of -1 is an offset of 4 GiB less 8 bytes and reads 0 with either descriptor.
// plane_load_at takes the BYTE offset of the element instead of its index, for a caller that carries the offset itself: bit
// 31 of an offset survives (an index loses it to the shift), and an offset with bit 31 set -- 2 GiB and more, past any
// descriptor; the byte offset -1 of an owner map that holds offsets among them -- reads 0 like the index -1 does.  The
// level kernels' residual of a pixel without an owner rests on that (gn_kernels.hip, pass 2).
template <typename T>
__device__ __forceinline__ double plane_load_at(__amdgpu_buffer_rsrc_t r, int byte_off, int soff = 0);
template <>
__device__ __forceinline__ double plane_load_at<double>(__amdgpu_buffer_rsrc_t r, int byte_off, int soff)
{
  const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, soff, 0);
  return __hiloint2double((int)v.y, (int)v.x);
}
template <>
__device__ __forceinline__ double plane_load_at<float>(__amdgpu_buffer_rsrc_t r, int byte_off, int soff)
{
  return (double)__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, soff, 0));
}
template <>
__device__ __forceinline__ double plane_load_at<__half>(__amdgpu_buffer_rsrc_t r, int byte_off, int soff)
{
  const unsigned short bits = __builtin_amdgcn_raw_buffer_load_b16(r, byte_off, soff, 0);
  return (double)__half2float(__ushort_as_half(bits));
}
template <typename T>
__device__ __forceinline__ double plane_load(__amdgpu_buffer_rsrc_t r, int idx, int soff = 0)
{
  return plane_load_at<T>(r, idx * (int)sizeof(T), soff);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 1/x to within one ulp: v_rcp_f64 seeds two Newton steps.  The IEEE-exact division sequence is
// 11 instructions, this is 5; the half-ulp it gives up is far below the fp64 noise floor of the sums
// that follow (tests/test_gpu_parity.py holds the poses to 1e-9 against the oracle's exact divisions).
// Contract, for 2^-1000 <= |x| <= 2^1000: STEPS = 2 is within one ulp of the IEEE quotient, STEPS = 1 has a relative
// error of at most 2^-48 (what its call sites quote); +-0, +-inf and NaN all give NaN (the seed is the IEEE quotient, the
// first step forms 0 x inf), which fails the callers' bounds tests.  tests/test_gpu_device_arith.py holds all three
// against IEEE division; DESIGN.md §4.1 has the measured figures.
template <int STEPS = 2>
__device__ __forceinline__ double fast_rcp(double x)
{
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(r, e, r);
  if (STEPS >= 2) {
    e = fma(-x, r, 1.0);
    r = fma(r, e, r);
  }
  return r;
}

// Entries of an owner map kept in HBM: (iteration tag << 21) | source index.  atomicMax still picks the largest
// source index among the entries of the running iteration, and every entry of an earlier one is smaller than any of
// them, so the map needs no reset between iterations (it is wiped per pair and whenever the 1023 tags start over).
constexpr int OWNER_TAG_SHIFT = 21;
constexpr int OWNER_INDEX_MASK = (1 << OWNER_TAG_SHIFT) - 1;      // levels of up to 2 097 151 pixels
constexpr int OWNER_TAG_PERIOD = 1023;

// Entries of an owner map kept in LDS for a level of n pixels and a workgroup of `threads` threads: whole 64-pixel chunks
// plus one round of the workgroup's chunks (see gn_level_kernel: pass 2 reads a chunk ahead, unguarded).  Even.
__host__ __device__ __forceinline__ constexpr int owner_lds_entries(int n, int threads)
{
  return ((n + 63) & ~63) + threads;
}

// a * b + c as ONE instruction on the 24-bit integer multiplier: row * width + column of a pixel index.  b is wave-uniform.
// What it saves is instructions, not a slow multiply (v_mul_lo_u32 issues at full rate on gfx950,
// profiles/r04_runs/valu_rate_probe.txt): written as row * W + column the compiler distributes the shift of the byte
// address over both terms -- multiply, two shifts, add3 -- where this and one shift-add do.  (HIP has __mul24 but no mad.)
__device__ __forceinline__ int mad24_uniform_b(int a, int b, int c)
{
  int r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
  return r;
}

// C round() -- half away from zero (...Analytic.h:297-298) -- for arguments > -0.5, which is all the bounds test lets
// through, in TWO instructions: floor(v + p) with p = 0.49999999999999994, the largest double below one half.  Exact, not
// approximately right (tests/test_oracle_properties.py checks every neighbour of every tie against exact arithmetic in a
// numpy emulation, tests/test_gpu_device_arith.py the same table through these two instructions on the device):
//   * a tie v = n + 0.5 gives n + 1 - 2^-54, which rounds to n + 1 (the next double below n + 1 is at least 2^-53 away for
//     n >= 1; for n = 0 the sum is halfway between 1 - 2^-53 and 1 and ties-to-even picks 1): round() says n + 1;
//   * the largest double below a tie, n + 0.5 - ulp, gives a sum that rounds to at most n + 1 - ulp: floor is n -- also
//     for 0.49999999999999994 itself, where the obvious floor(v + 0.5) goes wrong (the sum rounds up to 1.0);
//   * anything else is further than an ulp from a tie and the sum's rounding cannot carry it across an integer;
//   * (-0.5, 0) gives a sum in [0, 0.5): pixel 0, as round()'s -0.
// The trunc / fraction / compare / select / add form this replaces was five instructions per coordinate: 6 of the 50 of a
// pass-1 chunk (256 k -> 261 k alignments/s; the 5-level configuration, whose 40x30 level is vector-bound, +5 %).
__device__ __forceinline__ double round_half_up_from(double v)
{
  return floor(v + __hiloint2double(0x3fdfffff, (int)0xffffffff));
}

// Next pair of the work queue for the calling workgroup (one thread calls this), or n_pairs when everything is taken.
// With 8 queues, queue q serves the q-th contiguous eighth of the pair list and a workgroup starts with the queue of
// its XCD -- the hardware deals workgroups to the 8 XCDs round-robin, so blockIdx & 7 -- which keeps consecutive pairs
// of a sequence (they share a frame: the target of one is the source of the next) on one XCD's L2 at the same time;
// an empty queue sends the caller on to the next one.
// Every head has a cache line of its own (QUEUE_HEAD_STRIDE, round 3): the draws are device-scope atomics with a result
// and are served one after the other per line -- with all eight heads in ONE line the 8192 draws of a launch of short
// pairs stood in a single file (40x30 with the shipped thresholds, one iteration per pair: 1.05 -> 0.66 ms per launch;
// 80x60, every plane streamed once: 0.385 -> 0.32 ms).  Handing every workgroup its FIRST pair without an atomic on top
// of that was measured too and is not kept: nothing gained where the draws were the limit, -4 % with the shipped thresholds.
__device__ __forceinline__ int draw_pair(int *heads, int n_queues, int n_pairs)
{
  const int per = (n_pairs + n_queues - 1) / n_queues;
  int q = (int)(blockIdx.x & (unsigned)(n_queues - 1));                 // (n_queues is 1 or 8)
  for (int tries = 0; tries < n_queues; tries++) {
    const int first = q * per;
    const int size = first >= n_pairs ? 0 : (first + per > n_pairs ? n_pairs - first : per);
    if (size > 0) {
      const int t = atomicAdd(heads + q * QUEUE_HEAD_STRIDE, 1);
      if (t < size) return first + t;
    }
    q = (q + 1) & (n_queues - 1);
  }
  return n_pairs;
}

// Next pair for the calling workgroup: with GNLevelArgs::handover_in an index into the list the sliding-window launch of
// the level left behind (length at [n_pairs], final since that launch has ended) and the pair stored there; otherwise the
// plain queue.  n_pairs = nothing left.
__device__ __forceinline__ int draw_pair_any(const GNLevelArgs &A)
{
  if (!A.handover_in) return draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  const int count = __hip_atomic_load(&A.handover_in[A.n_pairs], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int i = atomicAdd(A.work_counter, 1);
  return i < count ? __hip_atomic_load(&A.handover_in[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : A.n_pairs;
}

// The calling thread puts `pair` on handover_out (after its state and iteration count have been stored; the kernel
// boundary makes all of it visible to the next launch).
__device__ __forceinline__ void handover_append(const GNLevelArgs &A, int pair)
{
  const int slot = atomicAdd(&A.handover_out[A.n_pairs], 1);
  A.handover_out[slot] = pair;
}

// v_writelane_b32: lane `lane` (wave-uniform) of `old` becomes `value` (wave-uniform); the other lanes keep theirs.
// clang has builtins for readlane / readfirstlane but none for writelane, so the LLVM intrinsic is declared by name
// (the device libraries do the same for intrinsics without a builtin).  Inline assembly is not an option: the lane
// select travels in M0 and the assembler's operand check then counts two scalar sources.
extern "C" __device__ int phovo_llvm_writelane_i32(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ int writelane_b32(int old, int value, int lane)
{
  return phovo_llvm_writelane_i32(value, lane, old);
}

// (row, column) of a lane's pixel, carried along as integer-valued doubles (exact), NW*64 pixels per step:
// column += step_c, and on running past the row end column -= W, row += 1.  W, step_r and step_r + 1 are small
// integers, so as doubles their low words are zero and each select is one v_cndmask on the high word.
struct RowColStep {
  double step_c, w;
  int hi_w, hi_step_r, hi_step_r1;
};
__device__ __forceinline__ RowColStep make_rowcol_step(int step_r, int step_c, int W)
{
  RowColStep s;
  s.step_c = (double)step_c;
  s.w = (double)W;
  s.hi_w = __double2hiint((double)W);
  s.hi_step_r = __double2hiint((double)step_r);
  s.hi_step_r1 = __double2hiint((double)(step_r + 1));
  return s;
}
__device__ __forceinline__ void rowcol_advance(double &cd, double &rd, const RowColStep &s)
{
  cd += s.step_c;
  const bool wrap = cd >= s.w;
  cd -= __hiloint2double(wrap ? s.hi_w : 0, 0);
  rd += __hiloint2double(wrap ? s.hi_step_r1 : s.hi_step_r, 0);
}

// (row, column) of pixel k from k itself, all in fp64: row = trunc((k + 0.5) / W), column = k - row * W.  Exact: k < 2^21
// and W are integers, (k + 0.5) / W lies at least 0.5 / W >= 2.4e-7 away from every integer while the fma below is off by
// less than (k / W) * 2^-52 < 1e-12, so the truncation cannot land on the wrong side; the column is an exact integer fma.
// (Every row boundary of 711 widths in exact rational arithmetic, tests/test_device_arith_cpu.py, and on the device,
// tests/test_gpu_device_arith.py.)
struct RowColFromIndex {
  double inv_w, half_inv_w, w;
};
__device__ __forceinline__ RowColFromIndex make_rowcol_from_index(int W)
{
  RowColFromIndex m;
  m.w = (double)W;
  m.inv_w = uniform_f64(1.0 / m.w);
  m.half_inv_w = 0.5 * m.inv_w;
  return m;
}
__device__ __forceinline__ void rowcol_from_index(double kd, const RowColFromIndex &m, double &cd, double &rd)
{
  rd = trunc(fma(kd, m.inv_w, m.half_inv_w));
  cd = fma(-rd, m.w, kd);
}

// The same for a cursor that may stand in front of the image (negative index): floor instead of trunc.
__device__ __forceinline__ void rowcol_from_index_floor(double kd, const RowColFromIndex &m, double &cd, double &rd)
{
  rd = floor(fma(kd, m.inv_w, m.half_inv_w));
  cd = fma(-rd, m.w, kd);
}

// The transposed butterfly over a wave's 64 lanes: 32 values per lane in, one total per lane out -- lane l returns the sum
// over the wave of value idx(l) = bit-reversed (l >> 1) (lanes l and l ^ 1 hold the same total).  Six stages: distance 32
// and 16 by lane swaps, 8 .. 1 by DPP moves; no stage goes through LDS.
__device__ __forceinline__ double wave_butterfly(double (&acc)[NRED], int lane)
{
  reduce_stage_swap<32, false>(acc);
  reduce_stage_swap<16, true>(acc);
  reduce_stage<8, 4, 8>(acc, lane);
  reduce_stage<4, 4, 4>(acc, lane);
  reduce_stage<2, 4, 2>(acc, lane);
  return acc[0] + dpp_f64<DPP_QUAD_XOR1>(acc[0]);
}

// A wave's 27 sums (+ the row count) folded over its 64 lanes and written to row `row` of s_red (transposed butterfly).
__device__ __forceinline__ void reduce_wave_to_row(double (&acc)[NRED], int lane, int row, double *s_red)
{
  const double total = wave_butterfly(acc, lane);
  const int idx = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 +
                  ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
  if ((lane & 1) == 0) s_red[row * NRED + idx] = total;
}

// Called by ONE whole wave behind the barrier that follows the butterflies' row stores: the 28 totals of the NROWS rows of
// s_red, in a fixed order -- lane l adds value (l & 31) over the first (l < 32) or the second half of the rows, row by row,
// and the halves meet in one exchange, first + second -- handed to every lane as h, g and the row count.
// The exchange is a lane swap (one v_permlane32_swap per dword); the 28 values then reach every lane through LDS: lanes
// 0 .. 31 store their totals over row 0 and all lanes read them back at wave-uniform addresses, 14 wide reads behind one
// another.  Nobody else touches s_red between the two barriers around this wave's section, and the store and the reads are
// the same wave's: a wave's LDS instructions execute and return in the order it issued them (one in-order queue per wave,
// which is also what lets lgkmcnt count them), so the reads see the store without a barrier or a wait between them.
// Through the crossbar it was 58 ds_bpermute_b32 (27 __shfl and the exchange), in wave 0's serial section.
// NROWS = 1 (one wave per pair): the row already is the total and is read in place.
template <int NROWS>
__device__ __forceinline__ void sum_rows_broadcast(int lane, double *s_red, double (&h)[21], double (&g)[6], int &n_valid)
{
  static_assert(NROWS == 1 || NROWS % 2 == 0, "the rows are summed in two halves");
  if constexpr (NROWS > 1) {
    const int j = lane & (NRED - 1);
    const int w0 = (lane >> 5) * (NROWS / 2);
    double r[NROWS / 2];
#pragma unroll
    for (int w2 = 0; w2 < NROWS / 2; w2++) r[w2] = s_red[(w0 + w2) * NRED + j];      // (the loads go out together)
    double v = 0.0;
#pragma unroll
    for (int w2 = 0; w2 < NROWS / 2; w2++) v += r[w2];
    // lanes 0 .. 31: own + partner's, as v += __shfl_xor(v, 32); the upper lanes' sums are not used
    const unsigned vlo = (unsigned)__double2loint(v), vhi = (unsigned)__double2hiint(v);
    const auto lo = __builtin_amdgcn_permlane32_swap(vlo, vlo, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(vhi, vhi, false, false);
    v = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
    if (lane < NRED) s_red[lane] = v;
  }
#pragma unroll
  for (int q = 0; q < 21; q++) h[q] = s_red[q];
#pragma unroll
  for (int i = 0; i < 6; i++) g[i] = s_red[21 + i];
  n_valid = (int)s_red[RED_VALID];
}

// The tail of a Gauss-Newton iteration on N parameters (the pose in the first six), by the one wave that solved: the state
// minus lambda * step, the finite test, the gradient norm, termination, the next iteration's pose constants, the flags.
template <int N>
__device__ __forceinline__ void update_and_terminate(int lane, const double (&step)[N], const double (&g)[N], double *s_state,
                                                     double *s_cst, int *s_ctl, double lambda, int max_iter,
                                                     double min_grad_norm, int iteration, int last_valid, double &last_gnorm)
{
  double st[N];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < N; i++) {
    st[i] = s_state[i] - lambda * step[i];                                            // :539
    finite = finite && finite_f64(st[i]);
  }
  double gn2 = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) gn2 += g[i] * g[i];
  const double gnorm = sqrt(gn2);                                                     // :380
  bool done = false;
  if (iteration + 1 >= max_iter) done = true;                                         // :383
  else if (gnorm < min_grad_norm) done = true;                                        // :388
  if (!finite) done = true;
  if (!done) write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, lane);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) s_state[i] = st[i];
    s_ctl[CTL_DONE] = done ? 1 : 0;
    if (!finite) s_ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_NONFINITE;
    if (last_valid < N) s_ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_RANK_DEFICIENT;
  }
  last_gnorm = gnorm;
}

// Called by ONE wave behind the barrier that follows reduce_wave_to_row: sum of the NROWS rows, solve, update, termination
// (as gn_level_kernel's tail); the caller closes with a barrier and reads s_ctl[CTL_DONE].
template <int NROWS>
__device__ __forceinline__ void sum_rows_solve_update(int lane, double *s_red, double *s_state, double *s_cst, int *s_ctl,
                                                      double lambda, int max_iter, double min_grad_norm,
                                                      int iteration, double &last_gnorm, int &last_valid)
{
  double h[21], g[6];
  sum_rows_broadcast<NROWS>(lane, s_red, h, g, last_valid);
  double step[6];
  solve6_ldlt(h, g, step);
  update_and_terminate<6>(lane, step, g, s_state, s_cst, s_ctl, lambda, max_iter, min_grad_norm, iteration, last_valid,
                          last_gnorm);
}

// Wave butterfly + cross-wave sum + solve + update + termination, as in gn_level_kernel's tail, for kernels
// that keep their 27 sums in `acc` in every wave.  Returns after the closing barrier; the caller reads s_ctl[CTL_DONE].
template <int NW>
__device__ __forceinline__ void reduce_solve_update(double (&acc)[NRED], int lane, int wave, double *s_red,
                                                    double *s_state, double *s_cst, int *s_ctl,
                                                    double lambda, int max_iter, double min_grad_norm,
                                                    int iteration, double &last_gnorm, int &last_valid)
{
  reduce_wave_to_row(acc, lane, wave, s_red);
  __syncthreads();
  if (wave == 0)
    sum_rows_solve_update<NW>(lane, s_red, s_state, s_cst, s_ctl, lambda, max_iter, min_grad_norm, iteration, last_gnorm,
                              last_valid);
  __syncthreads();
}

// One Jacobian row into a block of sums: the upper triangle of J^T W J (...Analytic.h:540), then J^T W r (:538); Jw = W J.
__device__ __forceinline__ void add_row(double (&acc)[NRED], const double (&Jw)[6], const double (&J)[6], const double res)
{
  int q = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int b = a; b < 6; b++) {
      acc[q] = fma(Jw[a], J[b], acc[q]);
      q++;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; a++) acc[21 + a] = fma(Jw[a], res, acc[21 + a]);
}
// W = identity: no weight and none of its instructions.
__device__ __forceinline__ void add_row(double (&acc)[NRED], const double (&J)[6], const double res) { add_row(acc, J, J, res); }

// One row of the analytic Jacobian on the reference-exact (nearest-scatter) path: the 2x6 warp Jacobian (:312-342)
// contracted with the image gradient (:348), for the source point (px, py, pz) and the target gradient (gxi, gyi).
// With Rt the rotation of the state, Pr = Rt * p = (Xr, Yr, Zr) and Jt = (J0, J1, J2) the row's three translation columns
//   temp25 = 1/Zd, Zd = z + Zr, Zr = py*temp1 + pz*temp2 - px*temp3,
//   Au = pz*temp4 + py*temp5 + px*temp11      [temp11 = temp15 + x carries the reference's bug, :253]
//   Bv = py*temp6 + pz*temp9 + px*temp14 + y
//   J0 = gx*fx*temp25, J1 = gy*fy*temp25, J2 = -(J0*Au + J1*Bv)*temp25.
// The three rotation columns are the derivatives of Pr by yaw, pitch and roll, each contracted with Jt.  The reference's
// generated code writes the three derivatives out one by one (:329-342); they are w_i x Pr for three axes that do not
// depend on the pixel -- yaw: e_z, pitch: (-sin yaw, cos yaw, 0), roll: Rt's first column (temp15, temp14, -temp3) -- and
// Jt . (w_i x Pr) = w_i . (Pr x Jt), so ONE cross product per pixel serves all three:
//   Xr  = Au - px*x      (Rt's first row times p: the bug term of temp11 cancels, as in the reference's own temp15 terms)
//   nYr = y - Bv         (-Yr; py*temp7 + pz*temp8 - px*temp14 of :329, since temp7 = -temp6, temp8 = -temp9)
//   c_z = J0*nYr + J1*Xr,  -c_x = nYr*J2 + Zr*J1,  c_y = Zr*J0 - Xr*J2
//   J3 = c_z,  J4 = cos(yaw)*c_y - sin(yaw)*c_x,  J5 = temp15*c_x + temp14*c_y - temp3*c_z:
// 13 fp64 instructions where the three derivatives and their contractions took 20, and neither temp16/17/24 nor
// temp21/temp7 are needed.  Au -- with the bug -- still enters J2 and through it J4 and J5, as in the reference; the
// identity is exact in real arithmetic and the grouping differs from the reference's by rounding only (5e-15 of |p| |Jt|).
// The cross product's fmas are spelled out: every kernel that carries the row forms it with the same grouping whatever
// the compiler contracts around it (the sliding-window kernel equals its exact fall-back bit for bit).  The constants
// come as values, so a kernel hands them over from wherever it keeps them -- scalar registers, vector registers (y, which
// meets another constant inside one fma), members of a block read from LDS; RCP_STEPS: fast_rcp's Newton steps for temp25.
//
// The row in the TWIST basis: q = (J0, J1, J2, c_z, c_y, -c_x), everything above up to the cross product.  The state-basis
// row is J = T q with a 6x6 matrix T of the state alone -- unit rows 0..3, row 4 = (0, 0, 0, 0, cos yaw, sin yaw), row 5 =
// (0, 0, 0, -temp3, temp14, -temp15) -- so J^T J = T (sum q q^T) T^T and J^T r = T (sum q r): the level kernels and the
// sliding-window kernel sum q and apply T once per iteration to the 27 totals (rotate_system below), which takes the five
// instructions of J4 and J5 out of every pixel.  A row weight (Huber) is a scalar per row and commutes with T.
template <int RCP_STEPS>
__device__ __forceinline__ void analytic_twist_row(const double px, const double py, const double pz, const double gxi,
                                                   const double gyi, const double fx, const double fy, const double x,
                                                   const double y, const double z, const double t1, const double t2,
                                                   const double t3, const double t4, const double t5, const double t6,
                                                   const double t9, const double t11, const double t14, double (&q)[6],
                                                   double &Zr)
{
  Zr = py * t1 + pz * t2 - px * t3;                                       // Zd - z
  const double t25 = fast_rcp<RCP_STEPS>(z + Zr);                         // :313
  const double Au = pz * t4 + py * t5 + px * t11;
  const double Bv = fma(py, t6, fma(pz, t9, fma(px, t14, y)));
  q[0] = (gxi * fx) * t25;                                                // :317
  q[1] = (gyi * fy) * t25;                                                // :322
  q[2] = -(q[0] * Au + q[1] * Bv) * t25;                                  // :325-326
  const double Xr = fma(-px, x, Au);
  const double nYr = y - Bv;
  q[5] = fma(Zr, q[1], nYr * q[2]);                                       // -c_x
  q[4] = fma(Zr, q[0], -(Xr * q[2]));                                     // c_y
  q[3] = fma(q[1], Xr, q[0] * nYr);                                       // c_z  :329-330
}

// The row in the state basis (the wide form and the evaluate kernels, whose J^T J is the state basis' by contract).
template <int RCP_STEPS>
__device__ __forceinline__ void analytic_row(const double px, const double py, const double pz, const double gxi, const double gyi,
                                             const double fx, const double fy, const double x, const double y, const double z,
                                             const double t1, const double t2, const double t3, const double t4, const double t5,
                                             const double t6, const double t9, const double t11, const double t14,
                                             const double t15, const double cosy, const double siny, double (&J)[6], double &Zr)
{
  analytic_twist_row<RCP_STEPS>(px, py, pz, gxi, gyi, fx, fy, x, y, z, t1, t2, t3, t4, t5, t6, t9, t11, t14, J, Zr);
  const double cyc = J[4], ncx = J[5];
  J[4] = fma(cosy, cyc, siny * ncx);                                      // :333-336
  J[5] = fma(-t3, J[3], fma(t14, cyc, -(t15 * ncx)));                     // :339-342
}

// The normal equations of the twist basis taken to the state basis: h, g in (the 21 + 6 totals of q q^T and q r, as
// solve6_ldlt lays them out) become the upper triangle of T h T^T and T g, T as above analytic_twist_row.  Lane-uniform
// work of the wave that solves, between sum_rows_broadcast and solve6_ldlt; the five constants are those of the state the
// rows were formed with.  Every product and fma is spelled out -- with the grouping of J4 and J5 in analytic_row -- so
// that every kernel rounds alike (the sliding-window kernel and its exact fall-back):
//   two(a, b)      = cos yaw * a + sin yaw * b                 row 4 of T on (., a, b):      2 roundings
//   three(a, b, c) = -temp3 * a + temp14 * b - temp15 * c      row 5 of T on (a, b, c):      3 roundings
// Entries among 0..3 are T's unit rows: copies.  Column 4 of rows 0..3 is two(), column 5 three(); the lower right 3x3
// block B = h[3..5][3..5] goes through B u and B v (u, v: rows 4 and 5 of T on indices 3..5), whose first entries are
// H34 and H35: H44 = u . B u, H45 = u . B v, H55 = v . B v.  42 fp64 instructions, the negations are operand modifiers.
// (tests/test_gpu_system_rotation.py holds every entry against exact rational arithmetic, with the rounding count of
// each entry's expression as written here.)
__device__ __forceinline__ void rotate_system(double (&h)[21], double (&g)[6], const double cosy, const double siny,
                                              const double t3, const double t14, const double t15)
{
  auto two = [&](const double a, const double b) { return fma(cosy, a, siny * b); };
  auto three = [&](const double a, const double b, const double c) { return fma(-t3, a, fma(t14, b, -(t15 * c))); };
  // B u and B v without their first entries (those are H34, H35 below), from the totals before any is overwritten
  const double bu4 = two(h[tri(4, 4)], h[tri(4, 5)]), bu5 = two(h[tri(4, 5)], h[tri(5, 5)]);
  const double bv4 = three(h[tri(3, 4)], h[tri(4, 4)], h[tri(4, 5)]), bv5 = three(h[tri(3, 5)], h[tri(4, 5)], h[tri(5, 5)]);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double a3 = h[tri(i, 3)], a4 = h[tri(i, 4)], a5 = h[tri(i, 5)];
    h[tri(i, 4)] = two(a4, a5);
    h[tri(i, 5)] = three(a3, a4, a5);
  }
  h[tri(4, 4)] = two(bu4, bu5);
  h[tri(4, 5)] = two(bv4, bv5);
  h[tri(5, 5)] = three(h[tri(3, 5)], bv4, bv5);                           // (h[3][5] is B v's first entry by now)
  const double g3 = g[3], g4 = g[4], g5 = g[5];
  g[4] = two(g4, g5);
  g[5] = three(g3, g4, g5);
}

// Host: a persistent kernel (one that draws its pairs from the work queue) on as many workgroups as stay resident, or one
// per pair if those are fewer.
template <typename Kernel, typename Args>
hipError_t launch_persistent(Kernel kernel, int n_pairs, int cu_count, int wgs_per_cu, int threads, size_t lds_bytes,
                             hipStream_t stream, const Args &args)
{
  const int resident = cu_count * wgs_per_cu;
  const dim3 grid((unsigned)(n_pairs < resident ? n_pairs : resident)), block((unsigned)threads);
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args);
  return hipGetLastError();
}

}  // namespace

}  // namespace phovo_hip
