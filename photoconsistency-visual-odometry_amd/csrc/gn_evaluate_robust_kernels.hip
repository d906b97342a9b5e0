// Evaluation of the weighted Gauss-Newton system of the ROBUST INVERSE-COMPOSITIONAL aligner at caller-supplied states
// (phovo_engine_evaluate_robust_pairs): per pair, in the TWIST basis (nu, omega),
//   delta = scale_factor * median |r|   (or the caller's own),      w = |r| <= delta ? 1 : delta / |r|,
//   information = sum w J J^T,  gradient = sum w J r,  cost = sum w r^2,  huber_cost = 2 sum rho_delta(r),
//   squared_cost = sum r^2,  rows,  outliers = rows with |r| > delta
// with exactly the rows, residual and Jacobian row of k_eval_inverse (gn_evaluate_inverse_kernels.hip) and the median rule
// and the weight of gn_level_kernel_inverse_robust (gn_inverse_robust_kernel.hip): it is the system that aligner solves in
// the FIRST iteration of a level started at that state, whose threshold is the median at the entry pose.
// TWIN: the pixel loop (Taps, warp_issue, the two-chunk pipeline around consume) stands in k_eval_inverse too; a change to
// it goes into both.  It is restated, not shared, so that objective 5's evaluate kernel stays what it was.
//
// The tile form of gn_evaluate_device.hpp (tiles, slabs, fixed summation orders: there), fp64 planes only.  The kernel
// boundary is the only synchronisation: no grid barrier, no spin loop, no loop whose trip count comes from memory.  The only
// atomics are integer adds (LDS and global), so the counts -- and with them every bit of the record -- do not depend on the
// order in which lanes, waves or tiles arrive.
//   k_eval_robust_hist    per tile: the residuals of its rows into a 4096-bin histogram in LDS; behind one barrier the
//                         non-zero words go into the pair's histogram in the workspace (cleared by the host in front of
//                         the launch).  Residuals crowd into a hundred or so low bins: a tile flushes at most as many words
//                         as it has distinct bins, where per-row global atomics of every tile would pile onto those words.
//   k_eval_robust_delta   one workgroup per pair: the median rule on the pair's histogram, m and delta to the workspace
//   k_eval_robust         k_eval_inverse with the weight; per tile one block of 32 sums (21 + 6 + rows + the three costs +
//                         outliers)
//   k_eval_robust_finish  fixed-order sum of the tile slabs into phovo_robust_system, one workgroup per pair
// With the caller's deltas only the last two run.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "gn_evaluate_device.hpp"

namespace phovo_hip {

namespace {

constexpr int ROBUST_BINS = 4096;
constexpr int RED_HUBER = 29;             // slots behind RED_COST (sum w r^2): 2 sum rho_delta(r), sum r^2, and the rows with
constexpr int RED_SQUARED = 30;           // |r| > delta, a count as exact as the row count
constexpr int RED_OUTLIERS = 31;
static_assert(RED_COST == 28 && RED_OUTLIERS == NRED - 1, "one block of NRED carries every sum, and is full");
static_assert(ET * 16 == ROBUST_BINS && ENW == 4, "a thread owns 16 bins; four wave totals");

// 256-thread workgroups per CU = waves per SIMD, chosen from the compiled kernels' register counts: DESIGN.md §23 has the
// figures.
constexpr int EVAL_ROBUST_HIST_WPS = 4;
constexpr int EVAL_ROBUST_WPS = 3;

// The bin of a residual, §22's six instructions.  No value indexes outside the 4096 words: fabs gives a number >= 0 or a
// NaN; in the first arm 0 <= q < 4096, so (int)q lies in 0 .. 4095; everything else -- |r| >= 1, an infinity, a NaN, for
// which the comparison is false -- takes the second arm, bin 4095.
__device__ __forceinline__ int robust_bin(double res)
{
  const double q = fabs(res) * 4096.0;
  return q < 4096.0 ? (int)q : ROBUST_BINS - 1;
}

// grid (tiles, pairs of the group).  g_hist: [pairs][4096] words, zero at the launch.
__global__ __launch_bounds__(ET, EVAL_ROBUST_HIST_WPS) void k_eval_robust_hist(const GNInverseEvalArgs A, unsigned *g_hist)
{
  __shared__ double s_cst[32];
  __shared__ unsigned s_hist[ROBUST_BINS];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int W = A.w, H = A.h;
#pragma unroll
  for (int j = 0; j < 16; j++) s_hist[j * ET + tid] = 0u;                 // (eval_pose_to_lds has the barrier)
  eval_pose_to_lds(A.states + (size_t)pair * 6, s_cst);
  const SampledPose P = sampled_pose_rt(s_cst);

  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(A.planes + (size_t)A.src[pair] * A.frame_bytes, A.frame_bytes);
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(A.planes + (size_t)A.tgt[pair] * A.frame_bytes, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_d = (int)A.plane_off[PLANE_D];
  const WarpFrame F = warp_frame(A);
  const RowColFromIndex rc_map = make_rowcol_from_index(W);

  // The two source values of the wave's four chunks go out first (k_eval_inverse's schedule without the gradient planes).
  double pzs[ECPW], i0s[ECPW];
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    pzs[j] = plane_load<double>(rS, k, o_d);
    i0s[j] = plane_load<double>(rS, k, o_i);
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
    if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {                       // rows only: nothing else is counted
      const double res = bilerp(w.ax, w.ay, w.tap[0], w.tap[1], w.tap[2], w.tap[3]) - i0s[j];
      __hip_atomic_fetch_add(&s_hist[robust_bin(res)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  };
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
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();                          // every count of the tile is in
  // Thread t flushes words t, t + 256, ...: the LDS reads touch 64 banks and the atomics of a wave go to one stretch of 256
  // bytes.  (Integer adds: the order in which the tiles arrive changes no count.)
  unsigned *hist = g_hist + (size_t)pair * ROBUST_BINS;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const unsigned c = s_hist[j * ET + tid];
    if (c != 0u) atomicAdd(hist + j * ET + tid, c);
  }
}

// One workgroup per pair: the median rule of the aligner on the pair's histogram; g_md[pair] = (m, delta).
// TWIN: the scan (sixteen bins per thread, six __shfl_up, four wave totals in LDS, the one thread that crosses `half`) stands
// in gn_level_kernel_inverse_robust too, word for word from `mine` on; a change to it goes into both.  The aligner reads
// swizzled LDS words and clears them; this kernel reads plain global ones, four 16-byte loads per thread.
__global__ __launch_bounds__(ET) void k_eval_robust_delta(const unsigned *g_hist, double scale, double *g_md)
{
  __shared__ int s_wave_total[ENW];
  const int pair = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  int cnt[16];
  {
    const uint4 *p = reinterpret_cast<const uint4 *>(g_hist + (size_t)pair * ROBUST_BINS + 16 * tid);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint4 v = p[j];
      cnt[4 * j] = (int)v.x; cnt[4 * j + 1] = (int)v.y; cnt[4 * j + 2] = (int)v.z; cnt[4 * j + 3] = (int)v.w;
    }
  }
  int mine = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) mine += cnt[j];
  int incl = mine;
#pragma unroll
  for (int d = 1; d < WAVE; d *= 2) {
    const int up = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += up;
  }
  if (lane == WAVE - 1) s_wave_total[wave] = incl;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  int below = 0, n = 0;
#pragma unroll
  for (int w2 = 0; w2 < ENW; w2++) {
    const int t = s_wave_total[w2];
    below += w2 < wave ? t : 0;
    n += t;
  }
  const int half = (n + 1) / 2;
  const int last = below + incl;            // the cumulative count through this thread's bins
  int before = last - mine;
  if (n == 0) {
    if (tid == 0) { g_md[2 * (size_t)pair] = 0.0; g_md[2 * (size_t)pair + 1] = scale * 0.0; }
  } else if (before < half && half <= last) {
    int kbin = 0, hk = 1;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (!found) {
        if (before + cnt[j] >= half) { found = true; kbin = 16 * tid + j; hk = cnt[j]; }
        else before += cnt[j];
      }
    }
    const double m = ((double)kbin + (double)(half - before) / (double)hk) * 0x1p-12;
    g_md[2 * (size_t)pair] = m;
    g_md[2 * (size_t)pair + 1] = scale * m;
  }
}

// grid (tiles, pairs of the group).  g_md[pair] = (m, delta): k_eval_robust_delta's, or the caller's delta behind a 0.
__global__ __launch_bounds__(ET, EVAL_ROBUST_WPS) void k_eval_robust(const GNInverseEvalArgs A, const double *__restrict__ g_md,
                                                                      double *g_part, int tiles)
{
  __shared__ double s_cst[32];
  __shared__ double s_red[ENW * NRED];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int W = A.w, H = A.h;
  eval_pose_to_lds(A.states + (size_t)pair * 6, s_cst);
  const SampledPose P = sampled_pose_rt(s_cst);
  const double delta = uniform_f64(g_md[2 * (size_t)pair + 1]);           // once per workgroup, into a scalar
  const double two_delta = 2.0 * delta, delta_sq = delta * delta;

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
  int n_rows = 0;                           // the wave's rows (wave-uniform)
  int n_out = 0;                            // THIS LANE's rows beyond delta: counted under the row mask, so per lane

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
    if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {                       // rows only: nothing else is counted
      const double res = bilerp(w.ax, w.ay, w.tap[0], w.tap[1], w.tap[2], w.tap[3]) - i0s[j];
      const double ar = fabs(res);
      const bool inlier = ar <= delta;      // (a NaN residual is neither inlier nor outlier: its weight is NaN)
      n_out += ar > delta ? 1 : 0;
      const double wgt = inlier ? 1.0 : delta / ar;
      double J[6], Jw[6];
      inverse_row(J, gxs[j], gys[j], w.px, w.py, w.pz, F.fx, F.fy);
#pragma unroll
      for (int i = 0; i < 6; i++) Jw[i] = wgt * J[i];
      acc[RED_COST] = fma(wgt * res, res, acc[RED_COST]);
      acc[RED_HUBER] = inlier ? fma(res, res, acc[RED_HUBER]) : fma(two_delta, ar, acc[RED_HUBER] - delta_sq);
      acc[RED_SQUARED] = fma(res, res, acc[RED_SQUARED]);
      add_row(acc, Jw, J, res);
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
  acc[RED_OUTLIERS] = (double)n_out;                                      // (the butterfly adds the lanes up: exact)
  tile_sums(acc, lane, wave, s_red, g_part, pair, tiles);
}

// phovo_robust_system from a slab total of one block per tile (finish_slab<NRED>), by the whole wave; delta and the median
// are copied from the workspace.
__device__ __forceinline__ void write_robust_system(phovo_robust_system *o, int lane, double v, const double *md)
{
  // lane (a, b) of the 6x6 matrix, 36 lanes: the upper-triangle slot of (min, max)(a, b).  Every shuffle runs in the
  // whole wave (its source lanes must be active).
  const int a = lane / 6, b = lane % 6;
  const int q = lane >= 36 ? 0 : (a <= b ? tri(a, b) : tri(b, a));
  const double h = __shfl(v, q, WAVE);
  if (lane < 36) o->information[lane] = h;
  const double g = __shfl(v, lane < 6 ? 21 + lane : 0, WAVE);
  if (lane < 6) o->gradient[lane] = g;
  const double rows = __shfl(v, RED_VALID, WAVE);
  const double cost = __shfl(v, RED_COST, WAVE);
  const double huber = __shfl(v, RED_HUBER, WAVE);
  const double squared = __shfl(v, RED_SQUARED, WAVE);
  const double outliers = __shfl(v, RED_OUTLIERS, WAVE);
  const bool finite = lane == RED_VALID || lane >= RED_OUTLIERS || finite_f64(v);     // (the two counts are always finite)
  const bool all_finite = __ballot(!finite) == 0ull;
  if (lane == 0) {
    o->cost = cost;
    o->huber_cost = huber;
    o->squared_cost = squared;
    o->median = md[0];
    o->delta = md[1];
    o->rows = (int32_t)rows;
    o->outliers = (int32_t)outliers;
    uint32_t flags = 0;
    if (rows < 6.0) flags |= PHOVO_PAIR_RANK_DEFICIENT;
    if (!all_finite) flags |= PHOVO_PAIR_NONFINITE;
    o->flags = flags;
    o->reserved = 0;
  }
}

// One workgroup per pair: the fixed-order sum of its slab, the system written from the upper triangle.
__global__ __launch_bounds__(ET) void k_eval_robust_finish(const double *g_part, int tiles, const double *g_md,
                                                            phovo_robust_system *out)
{
  finish_slab<NRED>(g_part, tiles, [&](int pair, int lane, double v) {
    write_robust_system(out + pair, lane, v, g_md + 2 * (size_t)pair);
  });
}

}  // namespace

hipError_t gn_eval_robust_pairs(const GNInverseEvalArgs &a, int n_pairs, double scale_factor, bool deltas_given,
                                unsigned *g_hist, double *g_md, double *g_part, phovo_robust_system *out, hipStream_t stream)
{
  if (n_pairs <= 0) return hipSuccess;
  const int tiles = gn_eval_tiles(a.n);
  if (!deltas_given) {
    if (!(scale_factor > 0.0)) return hipErrorInvalidValue;
    const hipError_t st = hipMemsetAsync(g_hist, 0, sizeof(unsigned) * ROBUST_BINS * (size_t)n_pairs, stream);
    if (st != hipSuccess) return st;
    hipLaunchKernelGGL(k_eval_robust_hist, dim3((unsigned)tiles, (unsigned)n_pairs), dim3(ET), 0, stream, a, g_hist);
    hipLaunchKernelGGL(k_eval_robust_delta, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_hist, scale_factor, g_md);
  }
  hipLaunchKernelGGL(k_eval_robust, dim3((unsigned)tiles, (unsigned)n_pairs), dim3(ET), 0, stream, a, g_md, g_part, tiles);
  hipLaunchKernelGGL(k_eval_robust_finish, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_part, tiles, g_md, out);
  return hipGetLastError();
}

}  // namespace phovo_hip
