// Evaluation of the Gauss-Newton system at caller-supplied states (phovo_engine_evaluate_pairs): per pair
//   information = J^T W J,  gradient = J^T W r,  cost = r^T W r,  rows = Jacobian rows filled
// with exactly the rows ComputeResidualsAndJacobians (...Analytic.h:191-367) fills at that state on one level: the depth
// gate (:280), the round() bounds test (:297-303), the scatter to the rounded target index with the last source pixel in
// raster order winning (:358), the target gradients read at the SOURCE index (:346-347) and the reference's Jacobian
// including its temp11 slip (:253) -- the matrix the aligner inverts (:538-540).  W is the identity, or with
// huber_delta > 0 the IRLS weights the aligner uses (1 or delta/|r|, from r at the state).
//
// The tile form of gn_evaluate_device.hpp (tiles, slabs, fixed summation orders: there):
//   k_eval_pass1   pose constants, warp, atomicMax into the owner map in HBM, per-chunk in-bounds ballots
//   k_eval_pass2   residual and Jacobian rows, 21 + 6 + 1 sums and the row count per tile into a slab; the owner slots
//                  are put back to -1.  No float atomics.
//   k_eval_finish  fixed-order sum of the tile slabs into phovo_pair_system, one workgroup per pair
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "gn_evaluate_device.hpp"

namespace phovo_hip {

namespace {

struct EvalPose {
  double cx, cyy, cz, r01, r02, r11, r12, t1, t2, t3, t4, t5, t6, t8, t11, t14, t15, cosy, siny;
};

// Wave 0 writes the pose constants of the pair's state into s_cst; every thread reads them back behind the barrier.
__device__ __forceinline__ EvalPose eval_pose(const double *st, double *s_cst)
{
  eval_pose_to_lds(st, s_cst);
  const double *c = s_cst;
  EvalPose p;
  p.cx = c[C_X]; p.cyy = c[C_Y]; p.cz = c[C_Z];
  p.r01 = c[C_R01]; p.r02 = c[C_R02]; p.r11 = c[C_R11]; p.r12 = c[C_R12];
  p.t1 = c[C_T1]; p.t2 = c[C_T2]; p.t3 = c[C_T3]; p.t4 = c[C_T4]; p.t5 = c[C_T5]; p.t6 = c[C_T6];
  p.t8 = c[C_T8]; p.t11 = c[C_T11]; p.t14 = c[C_T14]; p.t15 = c[C_T15];
  p.cosy = c[C_CY]; p.siny = c[C_SY];
  return p;
}

// grid (tiles, pairs of the group).  TD: storage type of the depth plane.
// TWIN: the warp / atomicMax / ballot body is k_wide_pass1's (gn_wide_kernels.hip) with the depth plane typed; the two
// must select the same rows, so a change to the warp semantics (:279-303, :358) goes into both.  k_eval_pass2's row
// arithmetic is k_wide_pass2's in the same way.
template <typename TD>
__global__ __launch_bounds__(ET) void k_eval_pass1(const GNEvalArgs A, int *g_owner, unsigned long long *g_mask)
{
  __shared__ double s_cst[32];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  const EvalPose P = eval_pose(A.states + (size_t)pair * 6, s_cst);
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<TD>(src_frame + A.plane_off[PLANE_D], n);
  int *owner = g_owner + (size_t)pair * (size_t)n;
  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const double min_d = A.min_depth, max_d = A.max_depth, dW = (double)W, dH = (double)H;
  const RowColFromIndex rc_map = make_rowcol_from_index(W);
  double pzs[ECPW];
#pragma unroll
  for (int j = 0; j < ECPW; j++)
    pzs[j] = plane_load<TD>(rD0, (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane);    // past the plane: 0
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int chunk = blockIdx.x * E_TILE_CHUNKS + j * ENW + wave;
    if (chunk >= A.n_chunks) break;
    const int k = chunk * WAVE + lane;
    bool inb = false;
    const double pz = pzs[j];                                             // :279
    if (k < n && min_d < pz && pz < max_d) {                              // :280
      double cd, rd;
      rowcol_from_index((double)k, rc_map, cd, rd);
      const double px = (cd - ox) * pz * ifx;                             // :282
      const double py = (rd - oy) * pz * ify;                             // :283
      const double X = ((P.t15 * px + P.r01 * py) + P.r02 * pz) + P.cx;   // :291
      const double Y = ((P.t14 * px + P.r11 * py) + P.r12 * pz) + P.cyy;
      const double Z = ((-P.t3 * px + P.t1 * py) + P.t2 * pz) + P.cz;
      const double iz = fast_rcp(Z);                                      // :294
      const double tc = (X * fx) * iz + ox;                               // :295
      const double tr = (Y * fy) * iz + oy;                               // :296
      const double rr = round(tr), rc = round(tc);                        // :297-298
      if (rr >= 0.0 && rr < dH && rc >= 0.0 && rc < dW) {                 // :302-303
        inb = true;
        atomicMax(&owner[__mul24((int)rr, W) + (int)rc], k);              // last raster writer wins  :358
      }
    }
    const unsigned long long m = __ballot(inb);
    if (lane == 0) g_mask[(size_t)pair * A.n_chunks + chunk] = m;
  }
}

// grid (tiles, pairs of the group).  TI / TD: storage type of the intensity and gradient planes / of the depth plane.
template <typename TI, typename TD>
__global__ __launch_bounds__(ET) void k_eval_pass2(const GNEvalArgs A, int *g_owner, const unsigned long long *g_mask,
                                                   double *g_part, int tiles)
{
  __shared__ double s_cst[32];
  __shared__ double s_red[ENW * NRED];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w;
  const EvalPose P = eval_pose(A.states + (size_t)pair * 6, s_cst);
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rI0 = plane_rsrc<TI>(src_frame + A.plane_off[PLANE_I], n);
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<TD>(src_frame + A.plane_off[PLANE_D], n);
  const __amdgpu_buffer_rsrc_t rI1 = plane_rsrc<TI>(tgt_frame + A.plane_off[PLANE_I], n);
  const __amdgpu_buffer_rsrc_t rGX = plane_rsrc<TI>(tgt_frame + A.plane_off[PLANE_GX], n);
  const __amdgpu_buffer_rsrc_t rGY = plane_rsrc<TI>(tgt_frame + A.plane_off[PLANE_GY], n);
  int *owner = g_owner + (size_t)pair * (size_t)n;
  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const double t9 = -P.t8;
  const double huber_delta = A.huber_delta;

  double acc[NRED];
#pragma unroll
  for (int j = 0; j < NRED; j++) acc[j] = 0.0;
  const RowColFromIndex rc_map = make_rowcol_from_index(W);
  int n_rows = 0;
  // every load of the wave's four chunks goes out first, the owner slots are reset behind the last one (as k_wide_pass2)
  int os[ECPW];
  unsigned long long ms[ECPW];
  double pzs[ECPW], gxs[ECPW], gys[ECPW], i1s[ECPW], i0s[ECPW];
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int chunk = blockIdx.x * E_TILE_CHUNKS + j * ENW + wave;
    const int k = chunk * WAVE + lane;
    os[j] = k < n ? owner[k] : -1;
    ms[j] = chunk < A.n_chunks ? g_mask[(size_t)pair * A.n_chunks + chunk] : 0ull;
  }
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    pzs[j] = plane_load<TD>(rD0, k);                                      // past the plane: 0
    gxs[j] = plane_load<TI>(rGX, k);                                      // gradient at the SOURCE index  :346-347
    gys[j] = plane_load<TI>(rGY, k);
    i1s[j] = plane_load<TI>(rI1, k);                                      // :309
  }
#pragma unroll
  for (int j = 0; j < ECPW; j++) i0s[j] = plane_load<TI>(rI0, os[j]);     // :308 (owner -1: past the plane -> 0)
#pragma unroll
  for (int j = 0; j < ECPW; j++) {                // every slot is read once and left at -1 for the next evaluation
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    if (k < n) owner[k] = -1;
  }
  // Two compiled copies of the row loop behind a wave-uniform branch: without Huber weights none of the extension's
  // instructions run.
  auto rows = [&](auto huber_tag) {
    constexpr bool HUBER = decltype(huber_tag)::value;
#pragma unroll
    for (int j = 0; j < ECPW; j++) {
      const int chunk = blockIdx.x * E_TILE_CHUNKS + j * ENW + wave;
      if (chunk >= A.n_chunks) break;
      const int k = chunk * WAVE + lane;
      const int o = os[j];
      const unsigned long long m = ms[j];
      n_rows += __builtin_popcountll(m);
      // r[k] is the residual of TARGET pixel k (:358): it enters the cost whenever k has an owner, and the gradient through
      // Jacobian row k, which belongs to SOURCE pixel k and is filled iff that pixel's warp passed (the ballot)
      const double res = o >= 0 ? i1s[j] - i0s[j] : 0.0;                  // :308-309,358
      double wgt = 1.0;
      if (HUBER) {                                  // the aligner's IRLS weight (gn_level_kernel, extension)
        const double ar = fabs(res);
        wgt = ar <= huber_delta ? 1.0 : huber_delta / ar;
      }
      if (o >= 0) acc[RED_COST] = fma(HUBER ? res * wgt : res, res, acc[RED_COST]);          // r^T W r
      if (!((m >> lane) & 1ull)) continue;
      const double pz = pzs[j];
      const double gxi = gxs[j], gyi = gys[j];
      double cd, rd;
      rowcol_from_index((double)k, rc_map, cd, rd);
      const double px = (cd - ox) * pz * ifx;
      const double py = (rd - oy) * pz * ify;
      // the analytic row of gn_level_kernel / k_wide_pass2 (gn_device.hpp, analytic_row), temp25 with both Newton steps
      double J[6], Zr;
      analytic_row<2>(px, py, pz, gxi, gyi, fx, fy, P.cx, P.cyy, P.cz, P.t1, P.t2, P.t3, P.t4, P.t5, P.t6, t9, P.t11, P.t14,
                      P.t15, P.cosy, P.siny, J, Zr);
      double Jw[6];
#pragma unroll
      for (int a = 0; a < 6; a++) Jw[a] = HUBER ? J[a] * wgt : J[a];
      add_row(acc, Jw, J, res);                                           // J^T W J  :540, J^T W r  :538
    }
  };
  if (huber_delta > 0.0) rows(std::true_type{}); else rows(std::false_type{});
  acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
  tile_sums(acc, lane, wave, s_red, g_part, pair, tiles);
}

// One workgroup per pair: the fixed-order sum of its slab, the system written from the upper triangle.
__global__ __launch_bounds__(ET) void k_eval_finish(const double *g_part, int tiles, phovo_pair_system *out)
{
  finish_slab<NRED>(g_part, tiles, [&](int pair, int lane, double v) { write_pair_system(out + pair, lane, v); });
}

template <typename TI, typename TD>
hipError_t eval_launch(const GNEvalArgs &a, int n_pairs, int tiles, int *g_owner, unsigned long long *g_mask,
                       double *g_part, phovo_pair_system *out, hipStream_t stream)
{
  const dim3 grid((unsigned)tiles, (unsigned)n_pairs);
  hipLaunchKernelGGL(k_eval_pass1<TD>, grid, dim3(ET), 0, stream, a, g_owner, g_mask);
  hipLaunchKernelGGL((k_eval_pass2<TI, TD>), grid, dim3(ET), 0, stream, a, g_owner, g_mask, g_part, tiles);
  hipLaunchKernelGGL(k_eval_finish, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_part, tiles, out);
  return hipGetLastError();
}

}  // namespace

int gn_eval_tiles(int n) { return eval_tiles(n); }

size_t gn_eval_slab_doubles_per_pair(int n) { return (size_t)gn_eval_tiles(n) * NRED; }

hipError_t gn_eval_pairs(const GNEvalArgs &a, int n_pairs, int storage, int *g_owner, unsigned long long *g_mask,
                         double *g_part, phovo_pair_system *out, hipStream_t stream)
{
  if (n_pairs <= 0) return hipSuccess;
  const int tiles = gn_eval_tiles(a.n);
  return with_storage_types(storage, [&](auto ti, auto td) {
    return eval_launch<decltype(ti), decltype(td)>(a, n_pairs, tiles, g_owner, g_mask, g_part, out, stream);
  });
}

}  // namespace phovo_hip
