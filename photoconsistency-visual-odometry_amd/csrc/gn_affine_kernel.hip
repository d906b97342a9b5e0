// PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE: forward-additive alignment with a per-pair gain and offset,
//   r_k = I1(u_k, v_k) - (1 + alpha) * I0_k - beta,
// estimated jointly with the pose.  The rows are those of the bilinear extension with the true warp Jacobian
// (gn_bilinear_kernel.hip, CORRECTED): the same source pixels in raster order, the same real-valued warp, the same "in bounds
// iff the nearest pixel is" test, the same twelve clamped taps of I1, GX1 and GY1 and the same six pose columns; two columns
// are appended, dr/dalpha = -I0_k and dr/dbeta = -1.  fp64 planes only, no Huber weights.
// One pass per iteration, no scatter and no owner map, any level size; one workgroup runs all iterations of a level for a pair.
// The form is gn_level_kernel_bilinear's (taps gathered into registers), with the taps read plane by plane -- twelve 8-byte
// loads per pixel -- and one chunk's taps in flight instead of two (see the pixel loop).
// Sums: 36 + 8 + the row count.  The new columns' structure is used: beside the 21 + 6 sums of the pose block a pixel adds
//   sum J_j I0, sum J_j (j < 6), sum I0^2, sum I0, sum r I0, sum r            (16 sums; sum 1 is the row count)
// and wave 0 puts the 8 x 8 system together from them (the signs of the two columns are applied there: exact).
// The sums travel as two blocks of NRED through the analytic kernels' butterfly and fixed-order cross-wave sum, so every
// summation order depends on the level size only.
#include <hip/hip_runtime.h>

#include "gn_sampled_device.hpp"

namespace phovo_hip {

namespace {

// second block of sums (slots of acc2)
enum { X_JI0 = 0, X_J = 6, X_I0I0 = 12, X_I0 = 13, X_RI0 = 14, X_R = 15 };

__host__ __device__ constexpr size_t affine_lds_bytes(int threads)
{
  return sizeof(double) * (32 + 8 + 2 * (size_t)(threads / WAVE) * NRED) + sizeof(int) * CTL_COUNT;
}

// Called by wave 0 behind the barrier that follows the two reduce_wave_to_row: sum of the NROWS rows of both blocks, the
// 8 x 8 system, solve, update, termination (sum_rows_solve_update with 8 in place of 6).
template <int NROWS>
__device__ __forceinline__ void affine_solve_update(int lane, const double *s_red, double *s_state, double *s_cst, int *s_ctl,
                                                    double lambda, int max_iter, double min_grad_norm, int iteration,
                                                    double &last_gnorm, int &last_valid)
{
  static_assert(NROWS % 2 == 0, "the rows are summed in two halves");
  double v = 0.0, u = 0.0;
  {
    const int j = lane & (NRED - 1);
    const int w0 = (lane >> 5) * (NROWS / 2);
#pragma unroll
    for (int w2 = 0; w2 < NROWS / 2; w2++) {
      v += s_red[(w0 + w2) * NRED + j];
      u += s_red[(NROWS + w0 + w2) * NRED + j];
    }
    v += __shfl_xor(v, 32, WAVE);
    u += __shfl_xor(u, 32, WAVE);
  }
  double h[36], g[NP];
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = i; j < 6; j++) h[tri8(i, j)] = __shfl(v, tri(i, j), WAVE);
    h[tri8(i, 6)] = -__shfl(u, X_JI0 + i, WAVE);
    h[tri8(i, 7)] = -__shfl(u, X_J + i, WAVE);
    g[i] = __shfl(v, 21 + i, WAVE);
  }
  const double rows = __shfl(v, RED_VALID, WAVE);
  h[tri8(6, 6)] = __shfl(u, X_I0I0, WAVE);
  h[tri8(6, 7)] = __shfl(u, X_I0, WAVE);
  h[tri8(7, 7)] = rows;
  g[6] = -__shfl(u, X_RI0, WAVE);
  g[7] = -__shfl(u, X_R, WAVE);
  last_valid = (int)rows;
  double step[NP];
  solve8_ldlt(h, g, step);
  update_and_terminate<NP>(lane, step, g, s_state, s_cst, s_ctl, lambda, max_iter, min_grad_norm, iteration, last_valid,
                           last_gnorm);
}

template <int T, int WPS>
__global__ __launch_bounds__(T, WPS) void gn_level_kernel_affine(const GNAffineArgs B)
{
  const GNLevelArgs &A = B.lv;
  constexpr int NW = T / WAVE;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PairLds L = pair_lds<NW, 2>(lds_raw);                          // state: the pose, alpha, beta; two blocks of sums

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  if (tid == 0) L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  for (;;) {                                // work queue, as in gn_level_kernel
  const int pair = pair_drawn(L);
  if (pair >= A.n_pairs) break;
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rI0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_I], n);
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_D], n);
  // one descriptor for the target frame; a plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];

  pair_begin(A, pair, wave, lane, L, [L, &B, pair] {
    L.state[6] = B.illum[(size_t)pair * 2];
    L.state[7] = B.illum[(size_t)pair * 2 + 1];
  });

  const WarpFrame F = warp_frame(A);
  const LaneWalk lw = lane_walk<NW>(wave, lane, W);

  int iteration = 0;
  double last_gnorm = 0.0;
  int last_valid = 0;
  while (true) {
    const SampledPose P = sampled_pose(L.cst);
    const double gain = 1.0 + uniform_f64(L.state[6]), beta = uniform_f64(L.state[7]);

    double acc[NRED], acc2[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = acc2[j] = 0.0;

    // Software pipeline over the wave's chunks.  gn_level_kernel_bilinear keeps TWO chunks' worth of taps in registers; with 44
    // sums instead of 27 that form needs more than the 256 registers two waves per SIMD leave a wave (30 spilled into the
    // pixel loop), so here ONE set of taps is in flight and the order is that of gn_level_kernel_bilinear_dma: the geometry of
    // chunk i+1 (its depth and source intensity requested a chunk earlier), then the three bilinear samples of chunk i (the
    // wait for its taps), then the twelve taps of chunk i+1 go out into the registers just freed, then the Jacobian row and
    // the 44 sums of chunk i run while they travel.  The arithmetic of a pixel is unchanged.
    struct Warped {
      double px, py, pz, Zr, t25, ax, ay, i0;
      int idx[4];                           // the clamped taps p00, p01, p10, p11: indices into a plane
      unsigned long long m;                 // lanes that are valid and land in bounds
    };
    double tap[12];                         // I1, GX1, GY1 at p00, p01, p10, p11 of the chunk whose taps are in flight
    int k = lw.k0;
    double cd = lw.cd0, rd = lw.rd0;
    double pz_next = plane_load<double>(rD0, k);                          // past the plane: 0
    double i0_next = plane_load<double>(rI0, k);
    auto warp = [&](Warped &w) {
      const double pz = pz_next;
      w.i0 = i0_next;
      pz_next = plane_load<double>(rD0, k + NW * WAVE);
      i0_next = plane_load<double>(rI0, k + NW * WAVE);
      clamped_taps(w.idx, warp_cell(w, warp_project(w, k, cd, rd, pz, P, F)), W, H);
      k += NW * WAVE;
      rowcol_advance(cd, rd, lw.step);
    };
    auto issue = [&](const Warped &w) {
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
          tap[t] = plane_load<double>(rT, w.idx[t], o_i);
          tap[4 + t] = plane_load<double>(rT, w.idx[t], o_gx);
          tap[8 + t] = plane_load<double>(rT, w.idx[t], o_gy);
        }
      }
    };
    auto sample3 = [&](const Warped &w, double (&smp)[3]) {               // -> the bilinear samples I1, GX1, GY1
#pragma unroll
      for (int c = 0; c < 3; c++) smp[c] = bilerp(w.ax, w.ay, tap[4 * c], tap[4 * c + 1], tap[4 * c + 2], tap[4 * c + 3]);
    };
    int n_rows = 0;
    auto consume = [&](const Warped &w, const double (&smp)[3]) {
      n_rows += __builtin_popcountll(w.m);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
        const double i0 = w.i0;
        const double res = (smp[0] - gain * i0) - beta;
        double J[6];
        pose_columns<true>(J, smp[1], smp[2], w, P, F.fx, F.fy);
        add_row(acc, J, res);
#pragma unroll
        for (int a = 0; a < 6; a++) {
          acc2[X_JI0 + a] = fma(J[a], i0, acc2[X_JI0 + a]);
          acc2[X_J + a] += J[a];
        }
        acc2[X_I0I0] = fma(i0, i0, acc2[X_I0I0]);
        acc2[X_I0] += i0;
        acc2[X_RI0] = fma(res, i0, acc2[X_RI0]);
        acc2[X_R] += res;
      }
    };
    {
      Warped w0, w1;
      double smp[3];
      int chunk = wave;                                                   // wave-uniform loop control throughout
      if (chunk < A.n_chunks) {
        warp(w0);
        issue(w0);
        for (;;) {
          chunk += NW;
          const bool more1 = chunk < A.n_chunks;
          if (more1) warp(w1);
          sample3(w0, smp);
          if (more1) issue(w1);
          consume(w0, smp);
          if (!more1) break;
          chunk += NW;
          const bool more0 = chunk < A.n_chunks;
          if (more0) warp(w0);
          sample3(w1, smp);
          if (more0) issue(w0);
          consume(w1, smp);
          if (!more0) break;
        }
      }
    }
    acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
    reduce_wave_to_row(acc, lane, wave, L.red);
    reduce_wave_to_row(acc2, lane, NW + wave, L.red);
    __syncthreads();
    if (wave == 0)
      affine_solve_update<NW>(lane, L.red, L.state, L.cst, L.ctl, A.lambda, A.max_iter, A.min_grad_norm, iteration,
                              last_gnorm, last_valid);
    __syncthreads();
    iteration++;
    if (L.ctl[CTL_DONE]) break;
  }
  if (tid == 0) {
    pair_report(A, pair, L, iteration, last_gnorm, last_valid, [L, &B, pair] {
      B.illum[(size_t)pair * 2] = L.state[6];
      B.illum[(size_t)pair * 2 + 1] = L.state[7];
    });
    L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

}  // namespace

// 256-thread workgroups per CU = waves per SIMD.  One chunk's taps (24 registers) and 44 fp64 sums (88) beside two chunks'
// geometry: DESIGN.md §14 has the register figures this geometry was chosen by.
constexpr int AFFINE_WPS = 2;

int gn_affine_wgs_per_cu() { return AFFINE_WPS; }
int gn_affine_lds_bytes() { return (int)affine_lds_bytes(256); }

hipError_t gn_launch_level_affine(const GNAffineArgs &b, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  if (!b.illum) return hipErrorInvalidValue;
  return launch_persistent(gn_level_kernel_affine<256, AFFINE_WPS>, b.lv.n_pairs, cu_count, AFFINE_WPS, 256,
                           affine_lds_bytes(256), stream, b);
}

}  // namespace phovo_hip
