// PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL: inverse-compositional photometric alignment (Baker & Matthews).
// The rows are the bilinear extension's (gn_sampled_device.hpp: the same source pixels in raster order, the same real-valued
// warp, the same "in bounds iff the nearest pixel is" test, the same four clamped taps of I1), the residual is
//   r_k = I1(u_k, v_k) - I0_k,
// but the Jacobian is taken on the SOURCE side, contracted with the source frame's own gradient planes, and depends on the
// source pixel alone: with p = (px, py, pz) the unprojected pixel and g = (GX0_k, GY0_k),
//   a = (g_x fx / pz, g_y fy / pz, -(a_0 px + a_1 py) / pz),     J_k = (a, p x a)      (twist order: nu, omega).
// A pixel and iteration cost four gathered taps (I1) and four coalesced loads (I0, D0, GX0, GY0) where the forward-additive
// aligners gather twelve taps and rebuild a pose-dependent row (pose_columns).
// The pose is carried as (R, t) inside a level: eigenPose(state) at the level's entry, then per iteration
//   xi = -lambda H^-1 g,   (R, t) <- (R E_R, R E_t + t),   (E_R, E_t) = Exp(xi) on SE(3),
// and the state (t, yaw, pitch, roll) is read off (R, t) when the level ends: the n x 6 state array stays the only thing that
// travels between the levels' launches.  fp64 planes only, no Huber weights.
// The form is gn_level_kernel_affine's: persistent, one 256-thread workgroup runs all iterations of a level for a pair, one
// pass per iteration, no scatter and no owner map, any level size.  A chunk's taps are 8 registers (not 24) and the sums
// are the 27 + 1 of the pose block alone, so TWO chunks' taps are in flight (see the pixel loop).
#include <hip/hip_runtime.h>

#include "gn_sampled_device.hpp"

namespace phovo_hip {

namespace {

// (E_R, E_t) = Exp(xi), xi = (nu, omega): E_R = I + A W + B W^2 (Rodrigues), E_t = (I + B W + C W^2) nu with W = [omega]x,
// A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3 = (1 - A) / th^2; below th^2 = 1e-8 the three come
// from their Taylor series through th^4 (the next term is below 1e-26 relative).  The whole wave calls this with a
// wave-uniform xi (the sines are pose_sincos_lane0's: its hand-written polynomials up to pi / 4, the device library's beyond).
__device__ __forceinline__ void se3_exp(const double (&xi)[6], int lane, double (&ER)[9], double (&Et)[3])
{
  const double wx = xi[3], wy = xi[4], wz = xi[5];
  const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
  const double th2 = xx + yy + zz;
  double A, B, C;
  if (th2 < 1e-8) {
    A = 1.0 - th2 * (1.0 / 6.0 - th2 * (1.0 / 120.0));
    B = 0.5 - th2 * (1.0 / 24.0 - th2 * (1.0 / 720.0));
    C = 1.0 / 6.0 - th2 * (1.0 / 120.0 - th2 * (1.0 / 5040.0));
  } else {
    const double th = sqrt(th2);
    double sn, cs, sh, ch, s2, c2;
    pose_sincos_lane0(th, 0.5 * th, th, lane, sn, cs, sh, ch, s2, c2);    // lane 1 worked on th / 2: lane 0 has both sines
    sn = uniform_f64(sn);                  // lane 0's, to every lane: everything below stays wave-uniform
    sh = uniform_f64(sh);
    A = sn / th;
    B = 2.0 * sh * sh / th2;               // 1 - cos th = 2 sin^2(th / 2): no cancellation (E_t has B W nu, first order in th)
    C = (1.0 - A) / th2;
  }
  const double xy = wx * wy, xz = wx * wz, yz = wy * wz;
  auto fill = [&](double (&M)[9], double a, double b) {                   // I + a W + b W^2,  W^2 = omega omega^T - th^2 I
    M[0] = 1.0 - b * (yy + zz); M[1] = b * xy - a * wz;     M[2] = b * xz + a * wy;
    M[3] = b * xy + a * wz;     M[4] = 1.0 - b * (xx + zz); M[5] = b * yz - a * wx;
    M[6] = b * xz - a * wy;     M[7] = b * yz + a * wx;     M[8] = 1.0 - b * (xx + yy);
  };
  fill(ER, A, B);
  double V[9];
  fill(V, B, C);
#pragma unroll
  for (int i = 0; i < 3; i++) Et[i] = V[3 * i] * xi[0] + V[3 * i + 1] * xi[1] + V[3 * i + 2] * xi[2];
}

// (yaw, pitch, roll) of a rotation matrix, the inverse of eigenPose: yaw = atan2(R10, R00), pitch = atan2(-R20,
// sqrt(R00^2 + R10^2)), roll = atan2(R21, R22).  Lanes 0, 1, 2 take one angle each (ONE atan2 issue); valid in lane 0.
__device__ __forceinline__ void euler_from_rotation_lane0(const double (&R)[9], int lane, double &yaw, double &pitch, double &roll)
{
  const double num = lane == 1 ? -R[6] : (lane == 2 ? R[7] : R[3]);
  const double den = lane == 1 ? sqrt(R[0] * R[0] + R[3] * R[3]) : (lane == 2 ? R[8] : R[0]);
  const double ang = atan2(num, den);
  yaw = ang;
  pitch = dpp_f64<DPP_QUAD_BCAST1>(ang);
  roll = dpp_f64<DPP_QUAD_BCAST2>(ang);
}

// Called by wave 0 behind the barrier that follows reduce_wave_to_row: the fixed-order sum of the NROWS rows, the 6 x 6
// solve, the twist, its exponential composed onto (R, t) in the constant block, termination (update_and_terminate's rule,
// with the finite test on (R, t)) and, when the level ends, the state read off (R, t).
template <int NROWS>
__device__ __forceinline__ void inverse_solve_compose(int lane, const PairLds L, double lambda, int max_iter,
                                                      double min_grad_norm, int iteration, double &last_gnorm, int &last_valid)
{
  double h[21], g[6];
  sum_rows_broadcast<NROWS>(lane, L.red, h, g, last_valid);
  double step[6], xi[6];
  solve6_ldlt(h, g, step);
#pragma unroll
  for (int i = 0; i < 6; i++) xi[i] = -lambda * step[i];
  double ER[9], Et[3], R[9], t[3], Rn[9], tn[3];
  se3_exp(xi, lane, ER, Et);
  rt_constants_read(L.cst, R, t);
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      Rn[3 * i + j] = R[3 * i] * ER[j] + R[3 * i + 1] * ER[3 + j] + R[3 * i + 2] * ER[6 + j];
      finite = finite && finite_f64(Rn[3 * i + j]);
    }
    tn[i] = (R[3 * i] * Et[0] + R[3 * i + 1] * Et[1] + R[3 * i + 2] * Et[2]) + t[i];
    finite = finite && finite_f64(tn[i]);
  }
  double gn2 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) gn2 += g[i] * g[i];
  const double gnorm = sqrt(gn2);
  bool done = false;
  if (iteration + 1 >= max_iter) done = true;
  else if (gnorm < min_grad_norm) done = true;
  if (!finite) done = true;
  if (done) {                                                             // (wave-uniform)
    double yaw, pitch, roll;
    euler_from_rotation_lane0(Rn, lane, yaw, pitch, roll);
    if (lane == 0) {
      const double nan = __hiloint2double(0x7ff80000, 0);
      L.state[0] = finite ? tn[0] : nan; L.state[1] = finite ? tn[1] : nan; L.state[2] = finite ? tn[2] : nan;
      L.state[3] = finite ? yaw : nan; L.state[4] = finite ? pitch : nan; L.state[5] = finite ? roll : nan;
    }
  }
  if (lane == 0) {
    rt_constants_write(L.cst, Rn, tn);
    L.ctl[CTL_DONE] = done ? 1 : 0;
    if (!finite) L.ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_NONFINITE;
    if (last_valid < 6) L.ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_RANK_DEFICIENT;
  }
  last_gnorm = gnorm;
}

template <int T, int WPS>
__global__ __launch_bounds__(T, WPS) void gn_level_kernel_inverse(const GNInverseArgs B)
{
  const GNLevelArgs &A = B.lv;
  constexpr int NW = T / WAVE;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PairLds L = pair_lds<NW>(lds_raw);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int W = A.w, H = A.h;
  if (tid == 0) L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  for (;;) {                                // work queue, as in gn_level_kernel
  const int pair = pair_drawn(L);
  if (pair >= A.n_pairs) break;
  // one descriptor per frame; a plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(A.planes + (size_t)A.src[pair] * A.frame_bytes, A.frame_bytes);
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(A.planes + (size_t)A.tgt[pair] * A.frame_bytes, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_d = (int)A.plane_off[PLANE_D];
  const int o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];

  pair_begin(A, pair, wave, lane, L);       // the block holds eigenPose(state): the (R, t) this level starts from

  const WarpFrame F = warp_frame(A);
  const LaneWalk lw = lane_walk<NW>(wave, lane, W);

  int iteration = 0;
  double last_gnorm = 0.0;
  int last_valid = 0;
  while (true) {
    const SampledPose P = sampled_pose_rt(L.cst);

    double acc[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = 0.0;

    // Software pipeline over the wave's chunks, two chunks' taps in flight: the geometry of chunk i+1 (its four source
    // values requested a chunk earlier) and its four taps go out BEFORE chunk i is consumed, so that behind the wait for
    // chunk i's taps the row and the 27 sums of chunk i run while the taps of chunk i+1 travel, and chunk i+2's go out
    // right behind them.  (Past the plane a prefetch reads the frame's next plane or, past the frame, 0: such a lane has
    // k >= n and the row mask drops it.)
    struct Warped {
      double px, py, pz, Zr, t25, ax, ay, i0, gx, gy;
      double tap[4];                        // I1 at p00, p01, p10, p11
      unsigned long long m;                 // lanes that are valid and land in bounds
    };
    int k = lw.k0;
    double cd = lw.cd0, rd = lw.rd0;
    double pz_next = plane_load<double>(rS, k, o_d), i0_next = plane_load<double>(rS, k, o_i);
    double gx_next = plane_load<double>(rS, k, o_gx), gy_next = plane_load<double>(rS, k, o_gy);
    auto warp_issue = [&](Warped &w) {
      const double pz = pz_next;
      w.i0 = i0_next; w.gx = gx_next; w.gy = gy_next;
      pz_next = plane_load<double>(rS, k + NW * WAVE, o_d);
      i0_next = plane_load<double>(rS, k + NW * WAVE, o_i);
      gx_next = plane_load<double>(rS, k + NW * WAVE, o_gx);
      gy_next = plane_load<double>(rS, k + NW * WAVE, o_gy);
      int idx[4];
      clamped_taps(idx, warp_cell(w, warp_project(w, k, cd, rd, pz, P, F)), W, H);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
        for (int t = 0; t < 4; t++) w.tap[t] = plane_load<double>(rT, idx[t], o_i);
      }
      k += NW * WAVE;
      rowcol_advance(cd, rd, lw.step);
    };
    int n_rows = 0;
    auto consume = [&](const Warped &w) {
      n_rows += __builtin_popcountll(w.m);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
        const double res = bilerp(w.ax, w.ay, w.tap[0], w.tap[1], w.tap[2], w.tap[3]) - w.i0;
        double J[6];
        inverse_row(J, w.gx, w.gy, w.px, w.py, w.pz, F.fx, F.fy);
        add_row(acc, J, res);
      }
    };
    {
      Warped w0, w1;
      int chunk = wave;                                                   // wave-uniform loop control throughout
      if (chunk < A.n_chunks) {
        warp_issue(w0);
        for (;;) {
          chunk += NW;
          const bool more1 = chunk < A.n_chunks;
          if (more1) warp_issue(w1);
          consume(w0);
          if (!more1) break;
          chunk += NW;
          const bool more0 = chunk < A.n_chunks;
          if (more0) warp_issue(w0);
          consume(w1);
          if (!more0) break;
        }
      }
    }
    acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
    reduce_wave_to_row(acc, lane, wave, L.red);
    __syncthreads();
    if (wave == 0)
      inverse_solve_compose<NW>(lane, L, A.lambda, A.max_iter, A.min_grad_norm, iteration, last_gnorm, last_valid);
    __syncthreads();
    iteration++;
    if (L.ctl[CTL_DONE]) break;
  }
  if (tid == 0) {
    pair_report(A, pair, L, iteration, last_gnorm, last_valid);
    L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

}  // namespace

// 256-thread workgroups per CU = waves per SIMD, chosen from the compiled kernel's register count: DESIGN.md §20 has the
// figures.
constexpr int INVERSE_WPS = 2;

int gn_inverse_wgs_per_cu() { return INVERSE_WPS; }
int gn_inverse_lds_bytes() { return (int)lds_fixed_bytes(256); }

hipError_t gn_launch_level_inverse(const GNInverseArgs &b, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  return launch_persistent(gn_level_kernel_inverse<256, INVERSE_WPS>, b.lv.n_pairs, cu_count, INVERSE_WPS, 256,
                           lds_fixed_bytes(256), stream, b);
}

}  // namespace phovo_hip
