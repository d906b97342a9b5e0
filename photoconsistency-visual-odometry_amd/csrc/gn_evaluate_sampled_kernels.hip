// Evaluation of the Gauss-Newton system of the SAMPLED aligners at caller-supplied states
// (phovo_engine_evaluate_sampled_pairs): per pair
//   information = J^T W J,  gradient = J^T W r,  cost = r^T W r,  rows = Jacobian rows filled
// with exactly the rows the bilinear extension (gn_bilinear_kernel.hip) and the affine-illumination objective
// (gn_affine_kernel.hip) fill at that state on one level: every source pixel in raster order that passes the strict depth
// gate and whose NEAREST target pixel is inside the image; I1, GX1 and GY1 sampled bilinearly from four taps with every
// index clamped to the image; residual and Jacobian row both belong to the source pixel (no scatter, no owner map).
// Three row kinds:
//   ROWS_SLIP       six columns of the reference's Jacobian, its temp11 slip (...Analytic.h:253) included
//   ROWS_CORRECTED  six columns of the true warp Jacobian
//   ROWS_AFFINE     the corrected six, dr/dalpha = -I0, dr/dbeta = -1, residual I1(u, v) - (1 + alpha) I0 - beta
// W is the identity, or on the six-column kinds with huber_delta > 0 the aligner's IRLS weights (1 or delta/|r|).
//
// The tile form of gn_evaluate_device.hpp (tiles, slabs, fixed summation orders: there) without gn_evaluate_kernels.hip's
// first pass (no atomics):
//   k_eval_sampled         pose constants, warp, twelve clamped taps per pixel gathered from the planes, the row's sums;
//                          per tile one block of 32 sums (21 + 6 + rows + cost) or, with eight columns, two (the affine
//                          kernel's second block: sum J_j I0, sum J_j, sum I0^2, sum I0, sum r I0, sum r)
//   k_eval_sampled_finish  fixed-order sum of the tile slabs into phovo_sampled_system, one workgroup per pair
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "gn_evaluate_device.hpp"

namespace phovo_hip {

namespace {

enum { ROWS_SLIP = 0, ROWS_CORRECTED = 1, ROWS_AFFINE = 2 };
// second block of sums (eight columns): the affine kernel's
enum { X_JI0 = 0, X_J = 6, X_I0I0 = 12, X_I0 = 13, X_RI0 = 14, X_R = 15 };

constexpr int blocks_of(int kind) { return kind == ROWS_AFFINE ? 2 : 1; }

// grid (tiles, pairs of the group).  TI / TD: storage type of the intensity and gradient planes / of the depth plane.
// The warp, the bounds test, the taps, the interpolation and the six columns are the aligners' (gn_sampled_device.hpp).
// TWIN: clamped_taps here against the tap policies that gn_level_kernel_bilinear and the fp64 gn_level_kernel_bilinear_dma
// keep for themselves (the header's note); they must name the same pixels wherever the row mask is set.
template <typename TI, typename TD, int KIND>
__global__ __launch_bounds__(ET) void k_eval_sampled(const GNSampledEvalArgs A, double *g_part, int tiles)
{
  constexpr int NB = blocks_of(KIND);
  constexpr bool AFFINE = KIND == ROWS_AFFINE;
  __shared__ double s_cst[32];
  __shared__ double s_red[NB * ENW * NRED];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  const double *st = A.states + (size_t)pair * A.state_dim;
  eval_pose_to_lds(st, s_cst);
  const SampledPose P = sampled_pose(s_cst);
  const double gain = AFFINE ? 1.0 + st[6] : 1.0, beta = AFFINE ? st[7] : 0.0;

  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rI0 = plane_rsrc<TI>(src_frame + A.plane_off[PLANE_I], n);
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<TD>(src_frame + A.plane_off[PLANE_D], n);
  // one descriptor for the target frame; a plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];
  const WarpFrame F = warp_frame(A);
  const double huber_delta = A.huber_delta;
  const RowColFromIndex rc_map = make_rowcol_from_index(W);

  double acc[NRED], acc2[NRED];            // (acc2: eight columns only)
#pragma unroll
  for (int j = 0; j < NRED; j++) acc[j] = acc2[j] = 0.0;
  int n_rows = 0;

  // depth and source intensity of the wave's four chunks go out first (past the plane: 0, which fails the depth gate)
  double pzs[ECPW], i0s[ECPW];
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    pzs[j] = plane_load<TD>(rD0, k);
    i0s[j] = plane_load<TI>(rI0, k);
  }

  double tap[12];                         // I1, GX1, GY1 at p00, p01, p10, p11 of the chunk whose taps are in flight
  auto warp = [&](Warped &w, int j) {
    warp_bilinear(w, (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane, pzs[j], P, F, W, H, rc_map);
  };
  auto issue = [&](const Warped &w) {
    if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
      for (int t = 0; t < 4; t++) {
        tap[t] = plane_load<TI>(rT, w.idx[t], o_i);
        tap[4 + t] = plane_load<TI>(rT, w.idx[t], o_gx);
        tap[8 + t] = plane_load<TI>(rT, w.idx[t], o_gy);
      }
    }
  };
  auto sample3 = [&](const Warped &w, double (&smp)[3]) {                 // -> the bilinear samples I1, GX1, GY1
#pragma unroll
    for (int c = 0; c < 3; c++) smp[c] = bilerp(w.ax, w.ay, tap[4 * c], tap[4 * c + 1], tap[4 * c + 2], tap[4 * c + 3]);
  };
  // Two compiled copies of the row loop behind a wave-uniform branch: without Huber weights none of the extension's
  // instructions run.  Order per chunk as in gn_level_kernel_affine: geometry of chunk j + 1, the three samples of chunk j
  // (the wait for its taps), the taps of chunk j + 1 go out into the registers just freed, then the row and its sums.
  auto rows = [&](auto huber_tag) {
    constexpr bool HUBER = decltype(huber_tag)::value;
    auto consume = [&](const Warped &w, const double (&smp)[3], double i0) {
      n_rows += __builtin_popcountll(w.m);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
        const double res = AFFINE ? (smp[0] - gain * i0) - beta : smp[0] - i0;
        double J[6];
        pose_columns<KIND != ROWS_SLIP>(J, smp[1], smp[2], w, P, F.fx, F.fy);
        double wgt = 1.0;
        if (HUBER) {                                // the aligner's IRLS weight
          const double ar = fabs(res);
          wgt = ar <= huber_delta ? 1.0 : huber_delta / ar;
        }
        acc[RED_COST] = fma(HUBER ? res * wgt : res, res, acc[RED_COST]); // r^T W r
        // (add_row's sums column by column, with the second block's between them: the order this kernel was compiled with)
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
          const double jw = HUBER ? J[a] * wgt : J[a];
#pragma unroll
          for (int b = a; b < 6; b++) {
            acc[q] = fma(jw, J[b], acc[q]);                               // J^T W J
            q++;
          }
          acc[21 + a] = fma(jw, res, acc[21 + a]);                        // J^T W r
          if (AFFINE) {
            acc2[X_JI0 + a] = fma(J[a], i0, acc2[X_JI0 + a]);
            acc2[X_J + a] += J[a];
          }
        }
        if (AFFINE) {
          acc2[X_I0I0] = fma(i0, i0, acc2[X_I0I0]);
          acc2[X_I0] += i0;
          acc2[X_RI0] = fma(res, i0, acc2[X_RI0]);
          acc2[X_R] += res;
        }
      }
    };
    Warped w[2];
    double smp[3];
    const int first = blockIdx.x * E_TILE_CHUNKS + wave;                  // wave-uniform loop control throughout
    if (first < A.n_chunks) {
      warp(w[0], 0);
      issue(w[0]);
#pragma unroll
      for (int j = 0; j < ECPW; j++) {
        const bool more = j + 1 < ECPW && first + (j + 1) * ENW < A.n_chunks;
        if (more) warp(w[(j + 1) & 1], j + 1);
        sample3(w[j & 1], smp);
        if (more) issue(w[(j + 1) & 1]);
        consume(w[j & 1], smp, i0s[j]);
        if (!more) break;
      }
    }
  };
  if (!AFFINE && huber_delta > 0.0) rows(std::true_type{}); else rows(std::false_type{});
  acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
  // tile_sums() for NB blocks: wave butterfly, then the four waves in fixed order, slab [pairs][tiles][NB][NRED]
  reduce_wave_to_row(acc, lane, wave, s_red);
  if (AFFINE) reduce_wave_to_row(acc2, lane, ENW + wave, s_red);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid < NB * NRED) {
    const int b = tid / NRED, j = tid & (NRED - 1);
    double v = 0.0;
#pragma unroll
    for (int w2 = 0; w2 < ENW; w2++) v += s_red[(b * ENW + w2) * NRED + j];
    g_part[(((size_t)pair * tiles + blockIdx.x) * NB + b) * NRED + j] = v;
  }
}

// One workgroup per pair: the fixed-order sum of its slab (finish_slab: 8 subsets of one block of sums, 4 of two blocks);
// the system is written from the upper triangle, with the signs of the affine columns applied here (exact).
template <int NB>
__global__ __launch_bounds__(ET) void k_eval_sampled_finish(const double *g_part, int tiles, phovo_sampled_system *out)
{
  constexpr int DIM = NB == 2 ? 8 : 6;
  // lanes 0..31: the first block of sums; 32..63: the second (eight columns)
  finish_slab<NB * NRED>(g_part, tiles, [&](int pair, int lane, double v) {
    phovo_sampled_system *o = out + pair;
    // lane (a, b) of the 8 x 8 record: the slot of (min, max)(a, b); rows and columns >= DIM are 0.  Every shuffle runs in
    // the whole wave (its source lanes must be active).
    const int a = min(lane >> 3, lane & 7), b = max(lane >> 3, lane & 7);
    int q = 0;
    bool negate = false, inside = b < DIM;
    if (b < 6) q = tri(a, b);
    else if (NB == 2) {
      if (a < 6) { q = NRED + (b == 6 ? X_JI0 : X_J) + a; negate = true; }
      else if (b == 6) q = NRED + X_I0I0;
      else q = a == 6 ? NRED + X_I0 : RED_VALID;
    }
    const double hs = __shfl(v, inside ? q : 0, WAVE);
    o->information[lane] = !inside ? 0.0 : (negate ? 0.0 - hs : hs);
    int qg = 0;
    if (lane < 6) qg = 21 + lane;
    else if (NB == 2 && lane < 8) qg = NRED + (lane == 6 ? X_RI0 : X_R);
    const double gs = __shfl(v, qg, WAVE);
    if (lane < 8) o->gradient[lane] = lane < 6 ? gs : (lane < DIM ? 0.0 - gs : 0.0);
    const double rows = __shfl(v, RED_VALID, WAVE);
    const double cost = __shfl(v, RED_COST, WAVE);
    const bool finite = finite_f64(v);                                  // (unused slots and lanes hold 0)
    const bool all_finite = __ballot(!finite) == 0ull;
    if (lane == 0) {
      o->cost = cost;
      o->rows = (int32_t)rows;
      uint32_t flags = 0;
      if (rows < (double)DIM) flags |= PHOVO_PAIR_RANK_DEFICIENT;
      if (!all_finite) flags |= PHOVO_PAIR_NONFINITE;
      o->flags = flags;
      o->dim = DIM;
      o->reserved = 0;
    }
  });
}

template <typename TI, typename TD>
hipError_t sampled_launch(const GNSampledEvalArgs &a, int n_pairs, int kind, int tiles, double *g_part,
                          phovo_sampled_system *out, hipStream_t stream)
{
  const dim3 grid((unsigned)tiles, (unsigned)n_pairs);
  if (kind == ROWS_CORRECTED)
    hipLaunchKernelGGL((k_eval_sampled<TI, TD, ROWS_CORRECTED>), grid, dim3(ET), 0, stream, a, g_part, tiles);
  else
    hipLaunchKernelGGL((k_eval_sampled<TI, TD, ROWS_SLIP>), grid, dim3(ET), 0, stream, a, g_part, tiles);
  hipLaunchKernelGGL(k_eval_sampled_finish<1>, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_part, tiles, out);
  return hipGetLastError();
}

}  // namespace

size_t gn_eval_sampled_slab_doubles_per_pair(int n, int dim) { return (size_t)gn_eval_tiles(n) * NRED * (dim == 8 ? 2 : 1); }

hipError_t gn_eval_sampled_pairs(const GNSampledEvalArgs &a, int n_pairs, int storage, bool corrected, double *g_part,
                                 phovo_sampled_system *out, hipStream_t stream)
{
  if (n_pairs <= 0) return hipSuccess;
  const int tiles = gn_eval_tiles(a.n);
  if (a.state_dim == 8) {                 // the affine-illumination rows: fp64 planes, no Huber weights
    if (storage != PHOVO_STORAGE_F64) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, (unsigned)n_pairs);
    hipLaunchKernelGGL((k_eval_sampled<double, double, ROWS_AFFINE>), grid, dim3(ET), 0, stream, a, g_part, tiles);
    hipLaunchKernelGGL(k_eval_sampled_finish<2>, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_part, tiles, out);
    return hipGetLastError();
  }
  if (a.state_dim != 6) return hipErrorInvalidValue;
  const int kind = corrected ? ROWS_CORRECTED : ROWS_SLIP;
  return with_storage_types(storage, [&](auto ti, auto td) {
    return sampled_launch<decltype(ti), decltype(td)>(a, n_pairs, kind, tiles, g_part, out, stream);
  });
}

}  // namespace phovo_hip
