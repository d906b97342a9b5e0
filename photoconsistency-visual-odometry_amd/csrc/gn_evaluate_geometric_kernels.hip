// Evaluation of the Gauss-Newton system of the photometric-geometric aligner at caller-supplied states
// (phovo_engine_evaluate_geometric_pairs): per pair the photometric block sum J_I J_I^T, sum J_I r_I,
// sum r_I^2 and the depth block sum J_D J_D^T, sum J_D r_D, sum r_D^2 SEPARATELY, and their entry-by-entry sum, with
// exactly the rows gn_level_kernel_geometric (gn_geometric_kernel.hip) fills at that state on one level.
// The photometric block is not computed here: it is k_eval_sampled's ROWS_CORRECTED system on fp64 planes without Huber
// weights (gn_eval_sampled_pairs, gn_evaluate_sampled_kernels.hip), run into its own slab and record.  This file adds the
// depth block, in that file's form (the tile form of gn_evaluate_device.hpp: tiles, slabs, fixed summation orders; no atomics):
//   k_eval_geometric_depth   pose constants, warp, the four clamped taps of the TARGET's depth per pixel, the tap gate, the
//                            residual gate, the depth row's sums; per tile one block of 32 sums (21 + 6 + depth rows +
//                            depth cost).  It reads D0 and D1 only: 16 algorithmic bytes per pixel.
//   k_eval_geometric_finish  fixed-order sum of the tile slabs, the sampled record beside it, information = photometric +
//                            depth with one add per entry, into phovo_geometric_system; one workgroup per pair
#include <hip/hip_runtime.h>

#include "gn_evaluate_device.hpp"

namespace phovo_hip {

namespace {

// slots of the block behind the 21 + 6 sums: the depth rows and sum r_D^2 stand where the other kernels keep their row
// count and cost
constexpr int RED_DEPTH_ROWS = RED_VALID, RED_DEPTH_COST = RED_COST;

// grid (tiles, pairs of the group).  fp64 planes.
// The warp, the bounds test, the taps, the interpolation and the six columns are the aligners' (gn_sampled_device.hpp).
// TWIN: the tap gate, the residual gate, dgx / dgy and rD are gn_level_kernel_geometric's (its `sample` and the head of
// `consume`); the two must select the same depth rows, so a change to those goes into both.
__global__ __launch_bounds__(ET) void k_eval_geometric_depth(const GNGeometricEvalArgs B, double *g_part, int tiles)
{
  const GNSampledEvalArgs &A = B.s;
  __shared__ double s_cst[32];
  __shared__ double s_red[ENW * NRED];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  const double *st = A.states + (size_t)pair * 6;
  eval_pose_to_lds(st, s_cst);
  const SampledPose P = sampled_pose(s_cst);

  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_D], n);
  // one descriptor for the target frame; its depth plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int o_d = (int)A.plane_off[PLANE_D];
  const WarpFrame F = warp_frame(A);
  const double min_d = F.min_d, max_d = F.max_d;
  const double sigma = B.depth_weight, gate = B.max_depth_residual;
  const bool gate_on = gate > 0.0;
  const RowColFromIndex rc_map = make_rowcol_from_index(W);

  double acc[NRED];
#pragma unroll
  for (int j = 0; j < NRED; j++) acc[j] = 0.0;
  int n_depth_rows = 0;

  // source depth of the wave's four chunks goes out first (past the plane: 0, which fails the depth gate)
  double pzs[ECPW];
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    pzs[j] = plane_load<double>(rD0, k);
  }

  struct Sampled {
    double d1, dgx, dgy;                  // the bilinear sample of D1 and the derivative of its interpolant
    bool taps_ok;                         // every D1 tap passes the depth gate
  };
  double tap[4];                          // D1 at p00, p01, p10, p11 of the chunk whose taps are in flight
  auto warp = [&](Warped &w, int j) {
    warp_bilinear(w, (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane, pzs[j], P, F, W, H, rc_map);
  };
  auto issue = [&](const Warped &w) {
    if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
      for (int t = 0; t < 4; t++) tap[t] = plane_load<double>(rT, w.idx[t], o_d);
    }
  };
  auto sample = [&](const Warped &w, Sampled &s) {
    const double ax = w.ax, ay = w.ay;
    s.d1 = bilerp(ax, ay, tap[0], tap[1], tap[2], tap[3]);
    const double p00 = tap[0], p01 = tap[1], p10 = tap[2], p11 = tap[3];
    s.dgx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10);
    s.dgy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01);
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 4; t++) ok = ok && (min_d < tap[t]) && (tap[t] < max_d);      // NaN fails
    s.taps_ok = ok;
  };
  auto consume = [&](const Warped &w, const Sampled &s) {
    const bool row = __builtin_amdgcn_inverse_ballot_w64(w.m);
    const double res_d = s.d1 - (P.cz + w.Zr);                          // D1(u, v) - Z'
    bool depth_row = row && s.taps_ok;
    if (gate_on) depth_row = depth_row && (fabs(res_d) <= gate);        // NaN fails
    n_depth_rows += __builtin_popcountll(__builtin_amdgcn_ballot_w64(depth_row));
    if (depth_row) {
      // the photometric row's six columns with the interpolant's derivative in place of the sampled gradients, and -dZ'/dp
      const double rD = sigma * res_d;
      double J[6];
      pose_columns<true>(J, sigma * s.dgx, sigma * s.dgy, w, P, F.fx, F.fy, sigma);
      // (add_row's sums, column by column: the products of column a, then its gradient entry -- the order this kernel was
      // compiled with; gn_evaluate_device.hpp's order schedules it differently)
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++) {
          acc[q] = fma(J[a], J[b], acc[q]);
          q++;
        }
        acc[21 + a] = fma(J[a], rD, acc[21 + a]);
      }
      acc[RED_DEPTH_COST] = fma(rD, rD, acc[RED_DEPTH_COST]);
    }
  };
  // Order per chunk as in k_eval_sampled: geometry of chunk j + 1, the sample of chunk j (the wait for its taps), the taps
  // of chunk j + 1 go out into the registers just freed, then the row and its sums.
  {
    Warped w[2];
    Sampled s;
    const int first = blockIdx.x * E_TILE_CHUNKS + wave;                  // wave-uniform loop control throughout
    if (first < A.n_chunks) {
      warp(w[0], 0);
      issue(w[0]);
#pragma unroll
      for (int j = 0; j < ECPW; j++) {
        const bool more = j + 1 < ECPW && first + (j + 1) * ENW < A.n_chunks;
        if (more) warp(w[(j + 1) & 1], j + 1);
        sample(w[j & 1], s);
        if (more) issue(w[(j + 1) & 1]);
        consume(w[j & 1], s);
        if (!more) break;
      }
    }
  }
  acc[RED_DEPTH_ROWS] = lane == 0 ? (double)n_depth_rows : 0.0;
  tile_sums(acc, lane, wave, s_red, g_part, pair, tiles);
}

// One workgroup per pair: the fixed-order sum of its depth slab (k_eval_sampled_finish's order); the photometric block
// comes from the pair's sampled record, and every entry of the record is written from the upper triangles, the sum with
// one add.
__global__ __launch_bounds__(ET) void k_eval_geometric_finish(const double *g_part, int tiles, const phovo_sampled_system *sampled,
                                                              phovo_geometric_system *out)
{
  finish_slab<NRED>(g_part, tiles, [&](int pair, int lane, double v) {      // lanes 0..31: the depth block's sums
    const phovo_sampled_system *ps = sampled + pair;
    phovo_geometric_system *o = out + pair;
    // lane (a, b) of the 6 x 6 records: the slot of (min, max)(a, b).  Every shuffle runs in the whole wave (its source lanes
    // must be active).
    const bool inside = lane < 36;
    const int ra = inside ? lane / 6 : 0, rb = inside ? lane - ra * 6 : 0;
    const int a = min(ra, rb), b = max(ra, rb);
    const double hd = __shfl(v, tri(a, b), WAVE);
    const double gd = __shfl(v, 21 + (lane < 6 ? lane : 0), WAVE);
    const double depth_rows = __shfl(v, RED_DEPTH_ROWS, WAVE);
    const double depth_cost = __shfl(v, RED_DEPTH_COST, WAVE);
    const bool finite = finite_f64(v);                                  // (unused slots and lanes hold 0)
    const bool depth_finite = __ballot(!finite) == 0ull;
    if (inside) {
      const double hi = ps->information[a * PHOVO_SYSTEM_MAX_DIM + b];
      o->photometric_information[lane] = hi;
      o->depth_information[lane] = hd;
      o->information[lane] = hi + hd;
    }
    if (lane < 6) {
      const double gi = ps->gradient[lane];
      o->photometric_gradient[lane] = gi;
      o->depth_gradient[lane] = gd;
      o->gradient[lane] = gi + gd;
    }
    if (lane == 0) {
      const int32_t rows = ps->rows;
      o->photometric_cost = ps->cost;
      o->depth_cost = depth_cost;
      o->rows = rows;
      o->depth_rows = (int32_t)depth_rows;
      uint32_t flags = 0;
      if (rows < 6) flags |= PHOVO_PAIR_RANK_DEFICIENT;
      if (!depth_finite || (ps->flags & PHOVO_PAIR_NONFINITE)) flags |= PHOVO_PAIR_NONFINITE;
      o->flags = flags;
      o->reserved = 0;
    }
  });
}

}  // namespace

hipError_t gn_eval_geometric_pairs(const GNGeometricEvalArgs &b, int n_pairs, double *g_part_sampled,
                                   phovo_sampled_system *sampled, double *g_part_depth, phovo_geometric_system *out,
                                   hipStream_t stream)
{
  if (n_pairs <= 0) return hipSuccess;
  if (b.s.state_dim != 6 || b.s.huber_delta != 0.0 || !(b.depth_weight > 0.0)) return hipErrorInvalidValue;
  // the photometric block: the corrected bilinear rows on fp64 planes, into the sampled slab and record
  const hipError_t st = gn_eval_sampled_pairs(b.s, n_pairs, PHOVO_STORAGE_F64, true, g_part_sampled, sampled, stream);
  if (st != hipSuccess) return st;
  const int tiles = gn_eval_tiles(b.s.n);
  hipLaunchKernelGGL(k_eval_geometric_depth, dim3((unsigned)tiles, (unsigned)n_pairs), dim3(ET), 0, stream, b, g_part_depth, tiles);
  hipLaunchKernelGGL(k_eval_geometric_finish, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_part_depth, tiles, sampled, out);
  return hipGetLastError();
}

}  // namespace phovo_hip
