// Evaluation of the Gauss-Newton system of the photometric-geometric aligner at caller-supplied states
// (phovo_engine_evaluate_geometric_pairs): per pair the photometric block sum J_I J_I^T, sum J_I r_I,
// sum r_I^2 and the depth block sum J_D J_D^T, sum J_D r_D, sum r_D^2 SEPARATELY, and their entry-by-entry sum, with
// exactly the rows gn_level_kernel_geometric (gn_geometric_kernel.hip) fills at that state on one level.
// The photometric block is not computed here: it is k_eval_sampled's ROWS_CORRECTED system on fp64 planes without Huber
// weights (gn_eval_sampled_pairs, gn_evaluate_sampled_kernels.hip), run into its own slab and record.  This file adds the
// depth block, in that file's form: a pair is cut into tiles of 16 64-pixel chunks, one 256-thread workgroup per tile, and
// the kernel boundary is the only synchronisation (no atomics, no grid barrier):
//   k_eval_geometric_depth   pose constants of the pair's state into LDS (write_pose_constants), warp, the four clamped taps
//                            of the TARGET's depth per pixel, the tap gate, the residual gate, the depth row's sums; per
//                            tile one block of 32 sums (21 + 6 + depth rows + depth cost).  It reads D0 and D1 only: 16
//                            algorithmic bytes per pixel.
//   k_eval_geometric_finish  fixed-order sum of the tile slabs, the sampled record beside it, information = photometric +
//                            depth with one add per entry, into phovo_geometric_system; one workgroup per pair
// The tile count and every summation order depend on the level size only: a pair's result is the same bit for bit
// whatever the batch, its position in it, or any setting of the engine.
#include <hip/hip_runtime.h>

#include "gn_device.hpp"
#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

constexpr int ET = 256;                 // threads per tile workgroup
constexpr int E_TILE_CHUNKS = 16;       // 64-pixel chunks per tile (1024 pixels), 4 per wave
constexpr int ENW = ET / WAVE;
constexpr int ECPW = E_TILE_CHUNKS / ENW;       // chunks per wave
// slots of the block behind the 21 + 6 sums: the depth rows stand where the other kernels keep their row count
constexpr int RED_DEPTH_ROWS = RED_VALID;
constexpr int RED_DEPTH_COST = 28;      // sum r_D^2
static_assert(RED_DEPTH_COST < NRED, "one block of NRED carries every sum");

// grid (tiles, pairs of the group).  fp64 planes.
// TWIN: the warp, the bounds test, the taps, both gates and the depth row are gn_level_kernel_geometric's (its `warp`,
// `sample` and the `if (depth_row)` block of `consume`); the two must select the same rows, so a change to those semantics
// goes into both.
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
  if (tid < WAVE) write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, tid);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  const double cx = uniform_f64(s_cst[C_X]), cyy = uniform_f64(s_cst[C_Y]), cz = uniform_f64(s_cst[C_Z]);
  const double r01 = uniform_f64(s_cst[C_R01]), r02 = uniform_f64(s_cst[C_R02]);
  const double r11 = uniform_f64(s_cst[C_R11]), r12 = uniform_f64(s_cst[C_R12]);
  const double t1 = uniform_f64(s_cst[C_T1]), t2 = uniform_f64(s_cst[C_T2]), t3 = uniform_f64(s_cst[C_T3]);
  const double t4 = uniform_f64(s_cst[C_T4]), t5 = uniform_f64(s_cst[C_T5]), t6 = uniform_f64(s_cst[C_T6]);
  const double t8 = uniform_f64(s_cst[C_T8]), t14 = uniform_f64(s_cst[C_T14]), t15 = uniform_f64(s_cst[C_T15]);
  const double t16 = uniform_f64(s_cst[C_T16]), t17 = uniform_f64(s_cst[C_T17]), t24 = uniform_f64(s_cst[C_T24]);
  const double cosy = uniform_f64(s_cst[C_CY]), siny = uniform_f64(s_cst[C_SY]);
  const double t7 = -t6, t9 = -t8, t21 = -t5;

  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_D], n);
  // one descriptor for the target frame; its depth plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int o_d = (int)A.plane_off[PLANE_D];
  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const double min_d = A.min_depth, max_d = A.max_depth;
  const double sigma = B.depth_weight, gate = B.max_depth_residual;
  const bool gate_on = gate > 0.0;
  const double wlim = (double)W - 0.5, hlim = (double)H - 0.5;
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

  struct Warped {
    double px, py, pz, Zr, t25, ax, ay;
    int idx[4];                           // the clamped taps p00, p01, p10, p11: indices into a plane
    unsigned long long m;                 // lanes that are valid and land in bounds
  };
  struct Sampled {
    double d1, dgx, dgy;                  // the bilinear sample of D1 and the derivative of its interpolant
    bool taps_ok;                         // every D1 tap passes the depth gate
  };
  double tap[4];                          // D1 at p00, p01, p10, p11 of the chunk whose taps are in flight
  auto warp = [&](Warped &w, int j) {
    const int k = (blockIdx.x * E_TILE_CHUNKS + j * ENW + wave) * WAVE + lane;
    const double pz = pzs[j];
    double cd, rd;
    rowcol_from_index((double)k, rc_map, cd, rd);
    const double px = (cd - ox) * pz * ifx;
    const double py = (rd - oy) * pz * ify;
    const double X = ((t15 * px + r01 * py) + r02 * pz) + cx;
    const double Y = ((t14 * px + r11 * py) + r12 * pz) + cyy;
    const double Zr = py * t1 + pz * t2 - px * t3;
    const double t25 = fast_rcp(cz + Zr);
    const double tc = (X * fx) * t25 + ox;
    const double tr = (Y * fy) * t25 + oy;
    // depth gate, and in bounds iff the NEAREST pixel is inside (NaN fails the comparisons)
    w.m = __builtin_amdgcn_ballot_w64(k < n) & __builtin_amdgcn_ballot_w64(min_d < pz) &
          __builtin_amdgcn_ballot_w64(pz < max_d) & __builtin_amdgcn_ballot_w64(tc > -0.5) &
          __builtin_amdgcn_ballot_w64(tc < wlim) & __builtin_amdgcn_ballot_w64(tr > -0.5) &
          __builtin_amdgcn_ballot_w64(tr < hlim);
    w.px = px; w.py = py; w.pz = pz; w.Zr = Zr; w.t25 = t25;
    const double fc = floor(tc), fr = floor(tr);
    w.ax = tc - fc;
    w.ay = tr - fr;
    // (lanes outside w.m: whatever the conversions give, clamped into the plane like the others; nobody uses their taps)
    const int ic = (int)fc, ir = (int)fr;
    const int r0w = __mul24(min(max(ir, 0), H - 1), W), r1w = __mul24(min(max(ir + 1, 0), H - 1), W);
    // clamp-to-edge taps (in the outer half-pixel band both taps of a row / a column are the edge pixel): every index
    // lies in [0, n)
    const int c0i = min(max(ic, 0), W - 1), c1i = min(max(ic + 1, 0), W - 1);
    w.idx[0] = r0w + c0i; w.idx[1] = r0w + c1i; w.idx[2] = r1w + c0i; w.idx[3] = r1w + c1i;
  };
  auto issue = [&](const Warped &w) {
    if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
      for (int t = 0; t < 4; t++) tap[t] = plane_load<double>(rT, w.idx[t], o_d);
    }
  };
  auto sample = [&](const Warped &w, Sampled &s) {
    const double ax = w.ax, ay = w.ay;
    s.d1 = (1.0 - ay) * ((1.0 - ax) * tap[0] + ax * tap[1]) + ay * ((1.0 - ax) * tap[2] + ax * tap[3]);
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
    const double res_d = s.d1 - (cz + w.Zr);                            // D1(u, v) - Z'
    bool depth_row = row && s.taps_ok;
    if (gate_on) depth_row = depth_row && (fabs(res_d) <= gate);        // NaN fails
    n_depth_rows += __builtin_popcountll(__builtin_amdgcn_ballot_w64(depth_row));
    if (depth_row) {
      const double px = w.px, py = w.py, pz = w.pz, Zr = w.Zr, t25 = w.t25;
      const double base = pz * t4 + py * t5 + px * t15;
      const double Au = base + cx;                                      // the true warp Jacobian (CORRECTED)
      const double Bv = py * t6 + pz * t9 + px * t14 + cyy;
      const double Cm = -py * t16 - pz * t17 - px * t24;                // dZ'/dpitch
      const double Dm = py * t2 - pz * t1;                              // dZ'/droll
      const double yawu = cyy - Bv, rollu = py * t4 + pz * t21, rollv = pz * t7 + py * t9;
      // the photometric row's six columns with the interpolant's derivative in place of the sampled gradients; dZ'/dp is
      // (0, 0, 1, 0, Cm, Dm), and since columns 4 and 5 take Cm and Dm times column 2, the -1 goes in there once
      const double rD = sigma * res_d;
      double J[6];
      J[0] = ((sigma * s.dgx) * fx) * t25;
      J[1] = ((sigma * s.dgy) * fy) * t25;
      J[2] = -(J[0] * Au + J[1] * Bv) * t25 - sigma;
      J[3] = J[0] * yawu + J[1] * base;
      J[4] = (J[0] * cosy + J[1] * siny) * Zr + Cm * J[2];
      J[5] = J[0] * rollu + J[1] * rollv + Dm * J[2];
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
  // tile sums: wave butterfly, then the four waves in fixed order
  reduce_wave_to_row(acc, lane, wave, s_red);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid < NRED) {
    double v = 0.0;
#pragma unroll
    for (int w2 = 0; w2 < ENW; w2++) v += s_red[w2 * NRED + tid];
    g_part[((size_t)pair * tiles + blockIdx.x) * NRED + tid] = v;
  }
}

// One workgroup per pair: thread (s, j) adds tiles s, s + 8, s + 16, ... of value j, then the eight subset sums are added in
// subset order (k_eval_sampled_finish's order); the photometric block comes from the pair's sampled record, and every entry
// of the record is written from the upper triangles, the sum with one add.
__global__ __launch_bounds__(ET) void k_eval_geometric_finish(const double *g_part, int tiles, const phovo_sampled_system *sampled,
                                                              phovo_geometric_system *out)
{
  constexpr int SUBSETS = ET / NRED;
  __shared__ double s_part[SUBSETS * NRED];
  const int pair = blockIdx.x, tid = threadIdx.x;
  {
    const int j = tid & (NRED - 1), sub = tid / NRED;
    const double *base = g_part + (size_t)pair * tiles * NRED + j;
    double v = 0.0;
#pragma unroll 4
    for (int t = sub; t < tiles; t += SUBSETS) v += base[(size_t)t * NRED];
    s_part[sub * NRED + j] = v;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid >= WAVE) return;
  const int lane = tid;
  double v = 0.0;                         // lanes 0..31: the depth block's sums
  if (lane < NRED) {
#pragma unroll
    for (int sub = 0; sub < SUBSETS; sub++) v += s_part[sub * NRED + lane];
  }
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
  const bool finite = fabs(v) <= 1.79769313486231570815e308;            // (unused slots and lanes hold 0)
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
