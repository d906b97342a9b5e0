// Evaluation of the Gauss-Newton system of the INVERSE-COMPOSITIONAL aligner at caller-supplied states
// (phovo_engine_evaluate_inverse_pairs): per pair, in the TWIST basis (nu, omega),
//   information = sum J J^T,  gradient = sum J r,  cost = sum r^2,  rows = Jacobian rows filled
// with exactly the rows gn_level_kernel_inverse (gn_inverse_kernel.hip) fills in the FIRST iteration of a level that starts
// from that state: (R, t) = eigenPose(state) as write_pose_constants leaves it in the block's twelve Rt slots, every source
// pixel in raster order that passes the strict depth gate and whose nearest target pixel is inside the image, I1 sampled
// bilinearly from four clamped taps, r = I1(u, v) - I0, and the source-side row J = (a, p x a) of inverse_row
// (gn_sampled_device.hpp) from the source frame's own gradient planes.  No weights: the objective has no Huber.
//
// The tile form of gn_evaluate_device.hpp (tiles, slabs, fixed summation orders: there), no atomics, fp64 planes only:
//   k_eval_inverse         pose constants, then per wave the four coalesced source values (D0, I0, GX0, GY0) of all its
//                          chunks, and per chunk the warp, four clamped taps of I1 gathered from the target frame and the
//                          row's sums, two chunks' taps in flight as in the aligner; per tile one block of 32 sums
//                          (21 + 6 + rows + cost)
//   k_eval_inverse_finish  fixed-order sum of the tile slabs into phovo_pair_system, one workgroup per pair
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "gn_evaluate_device.hpp"

namespace phovo_hip {

namespace {

// 256-thread workgroups per CU = waves per SIMD, chosen from the compiled kernel's register count: DESIGN.md §21 has the
// figures.
constexpr int EVAL_INVERSE_WPS = 3;

// grid (tiles, pairs of the group).  The warp, the bounds test, the taps, the interpolation and the row are the aligner's
// (gn_sampled_device.hpp); the pose is read as (R, t) by sampled_pose_rt, whose other members are 0: pose_columns is never
// reached from here.
__global__ __launch_bounds__(ET, EVAL_INVERSE_WPS) void k_eval_inverse(const GNInverseEvalArgs A, double *g_part, int tiles)
{
  __shared__ double s_cst[32];
  __shared__ double s_red[ENW * NRED];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int W = A.w, H = A.h;
  eval_pose_to_lds(A.states + (size_t)pair * 6, s_cst);
  const SampledPose P = sampled_pose_rt(s_cst);

  // one descriptor per frame; a plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(A.planes + (size_t)A.src[pair] * A.frame_bytes, A.frame_bytes);
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(A.planes + (size_t)A.tgt[pair] * A.frame_bytes, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_d = (int)A.plane_off[PLANE_D];
  const int o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];
  const WarpFrame F = warp_frame(A);
  const RowColFromIndex rc_map = make_rowcol_from_index(W);

  double acc[NRED];
#pragma unroll
  for (int j = 0; j < NRED; j++) acc[j] = 0.0;
  int n_rows = 0;

  // The four source values of the wave's four chunks go out first.  (Past the plane such a load reads the frame's next
  // plane or, past the frame, 0: that lane has k >= n and the row mask drops it.)
  double pzs[ECPW], i0s[ECPW], gxs[ECPW], gys[ECPW];
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    pzs[j] = plane_load<double>(rS, k, o_d);
    i0s[j] = plane_load<double>(rS, k, o_i);
    gxs[j] = plane_load<double>(rS, k, o_gx);
    gys[j] = plane_load<double>(rS, k, o_gy);
  }

  struct Taps {
    double px, py, pz, Zr, t25, ax, ay;
    double tap[4];                          // I1 at p00, p01, p10, p11
    unsigned long long m;                   // lanes that are valid and land in bounds
  };
  auto warp_issue = [&](Taps &w, int j) {
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    double cd, rd;
    rowcol_from_index((double)k, rc_map, cd, rd);
    int idx[4];
    clamped_taps(idx, warp_cell(w, warp_project(w, k, cd, rd, pzs[j], P, F)), W, H);
    if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
      for (int t = 0; t < 4; t++) w.tap[t] = plane_load<double>(rT, idx[t], o_i);
    }
  };
  auto consume = [&](const Taps &w, int j) {
    n_rows += __builtin_popcountll(w.m);
    if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
      const double res = bilerp(w.ax, w.ay, w.tap[0], w.tap[1], w.tap[2], w.tap[3]) - i0s[j];
      double J[6];
      inverse_row(J, gxs[j], gys[j], w.px, w.py, w.pz, F.fx, F.fy);
      acc[RED_COST] = fma(res, res, acc[RED_COST]);
      add_row(acc, J, res);
    }
  };
  // Per chunk: the geometry of chunk j + 1 and its four taps go out, then chunk j's interpolation, row and sums run behind
  // the wait for chunk j's taps alone.
  {
    Taps w[2];
    const int first = blockIdx.x * E_TILE_CHUNKS + wave;                  // wave-uniform loop control throughout
    if (first < A.n_chunks) {
      warp_issue(w[0], 0);
#pragma unroll
      for (int j = 0; j < ECPW; j++) {
        const bool more = j + 1 < ECPW && first + (j + 1) * ENW < A.n_chunks;
        if (more) warp_issue(w[(j + 1) & 1], j + 1);
        consume(w[j & 1], j);
        if (!more) break;
      }
    }
  }
  acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
  tile_sums(acc, lane, wave, s_red, g_part, pair, tiles);
}

// One workgroup per pair: the fixed-order sum of its slab, the system written from the upper triangle.
__global__ __launch_bounds__(ET) void k_eval_inverse_finish(const double *g_part, int tiles, phovo_pair_system *out)
{
  finish_slab<NRED>(g_part, tiles, [&](int pair, int lane, double v) { write_pair_system(out + pair, lane, v); });
}

}  // namespace

hipError_t gn_eval_inverse_pairs(const GNInverseEvalArgs &a, int n_pairs, double *g_part, phovo_pair_system *out,
                                 hipStream_t stream)
{
  if (n_pairs <= 0) return hipSuccess;
  const int tiles = gn_eval_tiles(a.n);
  hipLaunchKernelGGL(k_eval_inverse, dim3((unsigned)tiles, (unsigned)n_pairs), dim3(ET), 0, stream, a, g_part, tiles);
  hipLaunchKernelGGL(k_eval_inverse_finish, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_part, tiles, out);
  return hipGetLastError();
}

}  // namespace phovo_hip
