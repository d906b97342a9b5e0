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
// TWIN: the pixel loop (Warped, warp_issue, the two-chunk pipeline around consume) stands in gn_inverse_robust_kernel.hip and
// in gn_inverse_prior_kernel.hip (the form with a pose prior) too; a change to it goes into all three.
#include <hip/hip_runtime.h>

#include "gn_inverse_device.hpp"          // se3_exp, euler_from_rotation_lane0, inverse_solve_compose

namespace phovo_hip {

namespace {

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
