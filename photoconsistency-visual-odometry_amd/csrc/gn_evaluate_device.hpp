// The tile scaffold of the six "system at a given state" kernel files (gn_evaluate_kernels.hip,
// gn_evaluate_sampled_kernels.hip, gn_evaluate_geometric_kernels.hip, gn_evaluate_objective_kernels.hip,
// gn_evaluate_inverse_kernels.hip, gn_evaluate_robust_kernels.hip), included by those six and by nothing else.
//
// The form (the wide form's shape, gn_wide_kernels.hip): a pair is cut into tiles of 16 64-pixel chunks, one 256-thread
// workgroup per tile, grid (tiles, pairs of the group), and the kernel boundary is the only synchronisation (no grid
// barrier, no float atomics, nothing that can hang):
//   a tile kernel    wave 0 writes the pose constants of the pair's state into LDS (write_pose_constants: every sin/cos
//                    branch is the aligners'); wave w takes chunks w, w + 4, w + 8, w + 12 of the tile; every lane keeps
//                    one block of NRED sums (21 + 6 + the row count + the cost), or two; the tile's sums -- wave butterfly,
//                    then the four waves in wave order -- go into the tile's place in the pair's slab
//   a finish kernel  one workgroup per pair: thread (s, j) adds tiles s, s + S, s + 2 S, ... of value j, then the S subset
//                    sums are added in subset order, and one wave writes the record
// The tile count and every summation order depend on the level size only: a pair's record is the same bit for bit
// whatever the batch, its position in it, the group split, or any setting of the engine.  That promise rests on every
// kernel of the six files having this geometry and these orders, which is why they stand here once.
//
// Everything is __forceinline__ in an anonymous namespace, as in gn_device.hpp.  The first half (geometry, pose preamble,
// row sums, tile sums, finish) holds explicit fma() and plain adds only, so it means the same under
// `#pragma clang fp contract(off)` (gn_evaluate_objective_kernels.hip) and without; the bilinear warp at the end (and
// gn_sampled_device.hpp behind it) has products feeding adds and is for the files compiled with default contraction only
// (k_eval_inverse calls that warp's parts itself, as its aligner does).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "gn_sampled_device.hpp"

namespace phovo_hip {

namespace {

// ---- tile geometry ----------------------------------------------------------------------------------------------------
constexpr int ET = 256;                 // threads per tile workgroup
constexpr int E_TILE_CHUNKS = 16;       // 64-pixel chunks per tile (1024 pixels), 4 per wave
constexpr int ENW = ET / WAVE;
constexpr int ECPW = E_TILE_CHUNKS / ENW;       // chunks per wave
constexpr int RED_COST = 28;            // slot behind the row count (RED_VALID): r^T W r
static_assert(ENW * WAVE == ET && ECPW * ENW == E_TILE_CHUNKS, "whole waves, and every wave the same number of chunks");
static_assert(RED_VALID >= 27 && RED_VALID < RED_COST && RED_COST < NRED, "one block of NRED carries every sum");
static_assert(ET % NRED == 0 && (NRED & (NRED - 1)) == 0 && 2 * NRED <= WAVE, "the finish: whole subsets, one wave writes");

// 1024-pixel tiles of a level of n pixels (gn_eval_tiles): the slabs the host carves hold NRED doubles per tile and block.
constexpr int eval_tiles(int n) { return ((n + WAVE - 1) / WAVE + E_TILE_CHUNKS - 1) / E_TILE_CHUNKS; }

// ---- pose preamble ----------------------------------------------------------------------------------------------------
// Wave 0 writes the pose constants of the state st[0..5] into s_cst; every thread reads them behind the barrier.
__device__ __forceinline__ void eval_pose_to_lds(const double *st, double *s_cst)
{
  const int tid = threadIdx.x;
  if (tid < WAVE) write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, tid);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// (the row sums: add_row of gn_device.hpp)

// ---- tile sums --------------------------------------------------------------------------------------------------------
// The tile's block of sums: wave butterfly, then the four waves in fixed order, into the tile's place in the pair's slab
// ([pairs][tiles][NRED]).  (k_eval_sampled, which may carry two blocks, has its own.)
__device__ __forceinline__ void tile_sums(double (&acc)[NRED], int lane, int wave, double *s_red, double *g_part, int pair,
                                          int tiles)
{
  reduce_wave_to_row(acc, lane, wave, s_red);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < NRED) {
    double v = 0.0;
#pragma unroll
    for (int w2 = 0; w2 < ENW; w2++) v += s_red[w2 * NRED + tid];
    g_part[((size_t)pair * tiles + blockIdx.x) * NRED + tid] = v;
  }
}

// ---- finish -----------------------------------------------------------------------------------------------------------
// The fixed-order sum of the slab of NV values per tile of pair blockIdx.x, called by the whole workgroup: thread (s, j)
// adds tiles s, s + S, s + 2 S, ... of value j (S = ET / NV subsets); then, in wave 0 alone, lane j < NV adds the S subset
// sums in subset order, and the whole wave runs write(pair, lane, v): v is the total of value `lane`, 0 in lanes >= NV.
template <int NV, typename FWrite>
__device__ __forceinline__ void finish_slab(const double *g_part, int tiles, FWrite write)
{
  constexpr int SUBSETS = ET / NV;
  __shared__ double s_part[SUBSETS * NV];
  const int pair = blockIdx.x, tid = threadIdx.x;
  {
    const int j = tid & (NV - 1), sub = tid / NV;
    const double *base = g_part + (size_t)pair * tiles * NV + j;
    double v = 0.0;
#pragma unroll 4
    for (int t = sub; t < tiles; t += SUBSETS) v += base[(size_t)t * NV];
    s_part[sub * NV + j] = v;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid >= WAVE) return;
  const int lane = tid;
  double v = 0.0;
  if (lane < NV) {
#pragma unroll
    for (int sub = 0; sub < SUBSETS; sub++) v += s_part[sub * NV + lane];
  }
  write(pair, lane, v);
}

// phovo_pair_system from a slab total of one block per tile (finish_slab<NRED>), by the whole wave: k_eval_finish and
// k_obj_finish.
__device__ __forceinline__ void write_pair_system(phovo_pair_system *o, int lane, double v)
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
  const bool finite = lane >= RED_VALID || finite_f64(v);
  const bool all_finite = __ballot(!finite) == 0ull && finite_f64(cost);
  if (lane == 0) {
    o->cost = cost;
    o->rows = (int32_t)rows;
    uint32_t flags = 0;
    if (rows < 6.0) flags |= PHOVO_PAIR_RANK_DEFICIENT;
    if (!all_finite) flags |= PHOVO_PAIR_NONFINITE;
    o->flags = flags;
  }
}

// ---- host: plane storage -> <TI, TD> ---------------------------------------------------------------------------------
// launch(TI{}, TD{}) with the storage types of the intensity and gradient planes / of the depth plane (fp16 planes keep
// their depth in fp32); any other storage is hipErrorInvalidValue.
template <typename Launch>
hipError_t with_storage_types(int storage, Launch launch)
{
  switch (storage) {
    case PHOVO_STORAGE_F64: return launch(double{}, double{});
    case PHOVO_STORAGE_F32: return launch(float{}, float{});
    case PHOVO_STORAGE_F16: return launch(__half{}, float{});
    default: return hipErrorInvalidValue;
  }
}

// ---- bilinear warp (default contraction only: k_eval_sampled, k_eval_geometric_depth) --------------------------------
struct Warped {
  double px, py, pz, Zr, t25, ax, ay;
  int idx[4];                             // the clamped taps p00, p01, p10, p11: indices into a plane
  unsigned long long m;                   // lanes that are valid and land in bounds
};
// Source pixel k of depth pz through the pose, by the aligners' own warp (gn_sampled_device.hpp): the row's geometry, the
// bilinear weights and the four clamped taps.
__device__ __forceinline__ void warp_bilinear(Warped &w, int k, double pz, const SampledPose &P, const WarpFrame &F, int W, int H,
                                              const RowColFromIndex &rc_map)
{
  double cd, rd;
  rowcol_from_index((double)k, rc_map, cd, rd);
  clamped_taps(w.idx, warp_cell(w, warp_project(w, k, cd, rd, pz, P, F)), W, H);
}

}  // namespace

}  // namespace phovo_hip
