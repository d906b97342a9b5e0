// Evaluation of the trust-region and of the bi-objective system at caller-supplied states
// (phovo_engine_evaluate_objective_pairs): per pair
//   information = J^T J,  gradient = J^T r,  cost = r^T r,  rows
// with exactly the rows the aligner of the engine's objective fills at that state on one level:
//   trust region   the rows of gn_level_kernel_trust_region (gn_trust_region_kernel.hip): the real-valued
//                  bounds test, the target W trunc(v) + trunc(u), the largest source index landing on a target owning it,
//                  SampleLinear's taps and the exact warp Jacobian; rows = owned targets; cost = r^T r, which is TWICE
//                  Ceres's cost (1/2 sum r^2);
//   bi-objective   the 2N-row system of gn_level_kernel_biobjective (gn_biobjective_kernel.hip) with the
//                  reference's row collisions resolved as there; rows = contributing source pixels; cost = r^T r over the
//                  whole 2N residual vector, entries whose Jacobian row is empty included.
//
// The tile form of gn_evaluate_device.hpp (tiles, slabs, fixed summation orders: there), with gn_evaluate_kernels.hip's
// three kernels:
//   k_obj_pass1_*   pose constants, warp, atomicMax of the source index into the owner map in HBM, per-chunk ballots
//                   ("lands" / "contributes")
//   k_obj_pass2_*   residuals and rows, 21 + 6 sums, r^2 and the row count per tile into a slab.  No float atomics.
//   k_obj_finish    fixed-order sum of the tile slabs into phovo_pair_system, one workgroup per pair
//
// The owner maps hold -1 between calls.  Who puts them back differs:
//   trust region   pass 2.  Slot t is read by the landing pixels whose target is t -- possibly from several workgroups --
//                  and by nobody else.  Exactly one of them, the owner i = owner[t], finds its own index there, and only
//                  that thread stores -1.  Any other reader of t sees either i or -1; neither is its own index, so it
//                  takes the same decision (not the owner) whichever it sees.  Every slot that pass 1 raised has an owner
//                  that landed (its ballot bit is set), so every such slot is visited and restored.
//   bi-objective   a fill of its own behind pass 2.  Pass 2 of pixel i reads owner[i], owner[i/2] and owner[2i], entries of
//                  other tiles that other workgroups are still reading: a reset inside pass 2 would be a race.
#include <hip/hip_runtime.h>

// As gn_trust_region_kernel.hip: the warps are computed exactly as written, without contracting products into FMAs, so that
// the trust-region warp is the aligner's and the CPU checker's bit for bit.  The sums use explicit fma(), and so does
// everything this file takes from gn_evaluate_device.hpp (not its bilinear warp).
#pragma clang fp contract(off)

#include "gn_evaluate_device.hpp"
#include "gn_trust_region_device.hpp"

namespace phovo_hip {

namespace {

// ---- trust region ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tr_pose(const double *s_cst, double (&R)[9], double (&tv)[3])
{
  // Rt of eigenPose, the constants write_pose_constants stores (as gn_level_kernel_trust_region reads them)
  R[0] = uniform_f64(s_cst[C_T15]); R[1] = uniform_f64(s_cst[C_R01]); R[2] = uniform_f64(s_cst[C_R02]);
  R[3] = uniform_f64(s_cst[C_T14]); R[4] = uniform_f64(s_cst[C_R11]); R[5] = uniform_f64(s_cst[C_R12]);
  R[6] = -uniform_f64(s_cst[C_T3]); R[7] = uniform_f64(s_cst[C_T1]); R[8] = uniform_f64(s_cst[C_T2]);
  tv[0] = uniform_f64(s_cst[C_X]); tv[1] = uniform_f64(s_cst[C_Y]); tv[2] = uniform_f64(s_cst[C_Z]);
}

// grid (tiles, pairs of the group)
__global__ __launch_bounds__(ET) void k_obj_pass1_tr(const GNObjectiveEvalArgs A, int *g_owner, unsigned long long *g_mask)
{
  __shared__ double s_cst[32];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w;
  eval_pose_to_lds(A.states + (size_t)pair * 6, s_cst);
  double R[9], tv[3];
  tr_pose(s_cst, R, tv);
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(src_frame, A.frame_bytes);
  const int oD = (int)A.plane_off[PLANE_D];
  int *owner = g_owner + (size_t)pair * (size_t)n;
  const RowColFromIndex rc = make_rowcol_from_index(W);
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int chunk = blockIdx.x * E_TILE_CHUNKS + j * ENW + wave;
    if (chunk >= A.n_chunks) break;
    const int i = chunk * WAVE + lane;
    const double d = i < n ? plane_load<double>(rS, i, oD) : 0.0;
    const Warp w = warp_pixel((double)i, d, rc, A, R, tv);
    const bool ok = i < n && w.ok;                                  // 0 <= v < H and 0 <= u < W: the target is inside the map
    const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    if (lane == 0) g_mask[(size_t)pair * A.n_chunks + chunk] = m;
    if (ok) atomicMax(&owner[W * (int)w.v + (int)w.u], i);          // last raster writer wins  :255-257
  }
}

// grid (tiles, pairs of the group)
__global__ __launch_bounds__(ET) void k_obj_pass2_tr(const GNObjectiveEvalArgs A, int *g_owner,
                                                     const unsigned long long *g_mask, double *g_part, int tiles)
{
  __shared__ double s_cst[32];
  __shared__ double s_red[ENW * NRED];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  eval_pose_to_lds(A.states + (size_t)pair * 6, s_cst);
  double R[9], tv[3];
  tr_pose(s_cst, R, tv);
  const double cy = uniform_f64(s_cst[C_CY]), sy = uniform_f64(s_cst[C_SY]);
  const double cp = uniform_f64(s_cst[C_T24]);
  const double sp_sr = uniform_f64(s_cst[C_T16]), sp_cr = uniform_f64(s_cst[C_T17]);
  const double sr_cp = R[7], cr_cp = R[8];
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(src_frame, A.frame_bytes), rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int oI = (int)A.plane_off[PLANE_I], oD = (int)A.plane_off[PLANE_D];
  const int oGX = (int)A.plane_off[PLANE_GX], oGY = (int)A.plane_off[PLANE_GY];
  int *owner = g_owner + (size_t)pair * (size_t)n;
  const RowColFromIndex rc = make_rowcol_from_index(W);

  double acc[NRED];
#pragma unroll
  for (int j = 0; j < NRED; j++) acc[j] = 0.0;
#pragma unroll 1
  for (int j = 0; j < ECPW; j++) {
    const int chunk = blockIdx.x * E_TILE_CHUNKS + j * ENW + wave;
    if (chunk >= A.n_chunks) break;
    const unsigned long long mbits = g_mask[(size_t)pair * A.n_chunks + chunk];
    if (!((mbits >> lane) & 1ull)) continue;
    const int i = chunk * WAVE + lane;                              // (a set bit: i < n and the warp landed)
    const double d = plane_load<double>(rS, i, oD);
    const Warp w = warp_pixel((double)i, d, rc, A, R, tv);
    const int t = W * (int)w.v + (int)w.u;
    if (__hip_atomic_load(&owner[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != i) continue;   // a later pixel owns t
    __hip_atomic_store(&owner[t], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // the owner alone restores its slot
    // bilinear taps at (u, v) (SampleLinear, sample.h:53-99)
    int x1, x2, y1, y2;
    double wx, wy;
    linear_axis(w.u, W, x1, x2, wx);
    linear_axis(w.v, H, y1, y2, wy);
    const int k11 = y1 * W + x1, k12 = y1 * W + x2, k21 = y2 * W + x1, k22 = y2 * W + x2;
    const double i1 = bilinear(rT, oI, k11, k12, k21, k22, wx, wy);
    const double gxs = bilinear(rT, oGX, k11, k12, k21, k22, wx, wy);
    const double gys = bilinear(rT, oGY, k11, k12, k21, k22, wx, wy);
    const double res = i1 - plane_load<double>(rS, i, oI);                            // :262-263
    // d(u, v)/dx as gn_level_kernel_trust_region writes it
    const double iz = 1.0 / w.q2;
    const double du0 = A.fx * iz, dv1 = A.fy * iz;
    const double du2 = -A.fx * w.q0 * iz * iz, dv2 = -A.fy * w.q1 * iz * iz;
    const double ju = gxs * du0, jv = gys * dv1, jw = gxs * du2 + gys * dv2;
    const double dq2_pitch = -(cp * w.px + sp_sr * w.py + sp_cr * w.pz);
    const double dq0_roll = R[2] * w.py - R[1] * w.pz;
    const double dq1_roll = R[5] * w.py - R[4] * w.pz;
    const double dq2_roll = cr_cp * w.py - sr_cp * w.pz;
    const double J[6] = {ju, jv, jw, jv * w.a0 - ju * w.a1, (ju * cy + jv * sy) * w.a2 + jw * dq2_pitch,
                         ju * dq0_roll + jv * dq1_roll + jw * dq2_roll};
    add_row(acc, J, res);
    acc[RED_VALID] += 1.0;
    acc[RED_COST] = fma(res, res, acc[RED_COST]);
  }
  tile_sums(acc, lane, wave, s_red, g_part, pair, tiles);
}

// ---- bi-objective ---------------------------------------------------------------------------------------------------
struct BiPose {
  double cx, cyy, cz, r00, r01, r02, r10, r11, r12, r20, r21, r22;
};
__device__ __forceinline__ BiPose bi_pose(const double *s_cst)
{
  BiPose P;
  P.cx = uniform_f64(s_cst[C_X]); P.cyy = uniform_f64(s_cst[C_Y]); P.cz = uniform_f64(s_cst[C_Z]);
  P.r00 = uniform_f64(s_cst[C_T15]); P.r01 = uniform_f64(s_cst[C_R01]); P.r02 = uniform_f64(s_cst[C_R02]);
  P.r10 = uniform_f64(s_cst[C_T14]); P.r11 = uniform_f64(s_cst[C_R11]); P.r12 = uniform_f64(s_cst[C_R12]);
  // Rt (:275-291): row 2 is (-sin(pitch), temp1, temp2)
  P.r20 = -uniform_f64(s_cst[C_T3]); P.r21 = uniform_f64(s_cst[C_T1]); P.r22 = uniform_f64(s_cst[C_T2]);
  return P;
}

// grid (tiles, pairs of the group)
__global__ __launch_bounds__(ET) void k_obj_pass1_bi(const GNObjectiveEvalArgs A, int *g_owner, unsigned long long *g_mask)
{
  __shared__ double s_cst[32];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  eval_pose_to_lds(A.states + (size_t)pair * 6, s_cst);
  const BiPose P = bi_pose(s_cst);
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(src_frame, A.frame_bytes);
  const int oD = (int)A.plane_off[PLANE_D];
  int *owner = g_owner + (size_t)pair * (size_t)n;
  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const double min_d = A.min_depth, max_d = A.max_depth;
  const RowColFromIndex rc = make_rowcol_from_index(W);
#pragma unroll
  for (int j = 0; j < ECPW; j++) {
    const int chunk = blockIdx.x * E_TILE_CHUNKS + j * ENW + wave;
    if (chunk >= A.n_chunks) break;
    const int i = chunk * WAVE + lane;
    const double pz = i < n ? plane_load<double>(rS, i, oD) : 0.0;                  // :310
    double cd, rd;
    rowcol_from_index((double)i, rc, cd, rd);
    const double px = (cd - ox) * pz * ifx;                                         // :313
    const double py = (rd - oy) * pz * ify;                                         // :314
    const double X = P.r00 * px + P.r01 * py + P.r02 * pz + P.cx;                   // :322
    const double Y = P.r10 * px + P.r11 * py + P.r12 * pz + P.cyy;
    const double Z = P.r20 * px + P.r21 * py + P.r22 * pz + P.cz;
    const double iz = 1.0 / Z;                                                      // :325
    const double tc = (X * fx) * iz + ox;                                           // :326
    const double tr = (Y * fy) * iz + oy;                                           // :327
    // C round() (:328-329) for arguments > -0.5 (round_half_up_from), then the bounds (:333-334); NaN fails `> -0.5`
    const bool ok = i < n && min_d < pz && pz < max_d && tr > -0.5 && tc > -0.5 &&
                    round_half_up_from(tr) < (double)H && round_half_up_from(tc) < (double)W;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    if (lane == 0) g_mask[(size_t)pair * A.n_chunks + chunk] = m;
    if (ok) atomicMax(&owner[(int)round_half_up_from(tr) * W + (int)round_half_up_from(tc)], i);
  }
}

// grid (tiles, pairs of the group).  The thread of pixel k sees to
//   row k            its residual (the larger of owner[k] and, k even, owner[k/2]; a tie goes to depth) enters the cost; if
//                    k > 0 and pixel k contributes, Jint(k) with that residual enters the system;
//   row 2k, 2k >= N  its residual (the depth write of owner[k]) enters the cost; if pixel k contributes, Jdep(k) with it;
//   row 2k, 2k < N   if pixel k contributes and not (2k > 0 and pixel 2k contributes): Jdep(k) with the residual of row 2k
//                    (the larger of owner[2k] and owner[k]); that residual's square is counted by the thread of pixel 2k.
// So every one of the 2N residual entries is counted once (odd rows at or above N have no writer), and every Jacobian row
// once, as gn_level_kernel_biobjective's pass 2 adds them.
__global__ __launch_bounds__(ET) void k_obj_pass2_bi(const GNObjectiveEvalArgs A, const int *g_owner,
                                                     const unsigned long long *g_mask, double *g_part, int tiles)
{
  __shared__ double s_cst[32];
  __shared__ double s_red[ENW * NRED];
  const int pair = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w;
  eval_pose_to_lds(A.states + (size_t)pair * 6, s_cst);
  const BiPose P = bi_pose(s_cst);
  const double t1 = P.r21, t2 = P.r22, t3 = -P.r20;
  // (the constants only the Jacobians use stay in vector registers: the kernel has them to spare and no scalar one spills)
  const double t4 = s_cst[C_T4], t5 = s_cst[C_T5], t6 = s_cst[C_T6];
  const double t8 = s_cst[C_T8], t14 = P.r10, t15 = P.r00;
  const double t16 = s_cst[C_T16], t17 = s_cst[C_T17], t24 = s_cst[C_T24];
  const double cosy = s_cst[C_CY], siny = s_cst[C_SY];
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(src_frame, A.frame_bytes), rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int oI = (int)A.plane_off[PLANE_I], oD = (int)A.plane_off[PLANE_D];
  const int oGX = (int)A.plane_off[PLANE_GX], oGY = (int)A.plane_off[PLANE_GY];
  const int oDGX = (int)A.dgx_off, oDGY = (int)A.dgy_off;
  const int *owner = g_owner + (size_t)pair * (size_t)n;
  const unsigned long long *mask = g_mask + (size_t)pair * A.n_chunks;
  // gain = mean(target gray) / mean(target depth) (:300), resident for the target frame
  const double gain = uniform_f64(*reinterpret_cast<const double *>(tgt_frame + A.gain_off));
  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const RowColFromIndex rc = make_rowcol_from_index(W);

  // the residual of row m: intensity candidate o_int (its target is the row), depth candidate o_dep (its target is m/2)
  auto residual = [&](int m, int o_int, int o_dep) {
    double res = 0.0;
    if (o_dep >= 0 && o_dep >= o_int) res = gain * (plane_load<double>(rT, m >> 1, oD) - plane_load<double>(rS, o_dep, oD));
    else if (o_int >= 0) res = plane_load<double>(rT, m, oI) - plane_load<double>(rS, o_int, oI);
    return res;
  };

  double acc[NRED];
#pragma unroll
  for (int j = 0; j < NRED; j++) acc[j] = 0.0;
  int n_contrib = 0;
#pragma unroll 1
  for (int j = 0; j < ECPW; j++) {
    const int chunk = blockIdx.x * E_TILE_CHUNKS + j * ENW + wave;
    if (chunk >= A.n_chunks) break;
    const unsigned long long mbits = mask[chunk];
    if (lane == 0) n_contrib += __builtin_popcountll(mbits);
    const int i = chunk * WAVE + lane;
    if (i >= n) continue;
    const bool contributes = (mbits >> lane) & 1ull;
    const int i2 = 2 * i;
    const int o_i = owner[i];
    const int o_half = (i & 1) ? -1 : owner[i >> 1];
    const int o_i2 = i2 < n ? owner[i2] : -1;
    const bool c2 = i2 < n && ((mask[i2 >> 6] >> (i2 & 63)) & 1ull);
    const double res_i = residual(i, o_i, o_half);
    acc[RED_COST] = fma(res_i, res_i, acc[RED_COST]);
    const bool row2_mine = i2 >= n || (contributes && !(i2 > 0 && c2));      // this thread needs the residual of row 2i
    const double res_i2 = row2_mine ? residual(i2, o_i2, o_i) : 0.0;
    if (i2 >= n) acc[RED_COST] = fma(res_i2, res_i2, acc[RED_COST]);
    if (!contributes) continue;
    const double pz = plane_load<double>(rS, i, oD);
    const double gx = plane_load<double>(rT, i, oGX), gy = plane_load<double>(rT, i, oGY);     // at the SOURCE index  :424-425
    const double dgx = plane_load<double>(rT, i, oDGX), dgy = plane_load<double>(rT, i, oDGY); // :430-431
    double cd, rd;
    rowcol_from_index((double)i, rc, cd, rd);
    const double px = (cd - ox) * pz * ifx;
    const double py = (rd - oy) * pz * ify;
    const double X = P.r00 * px + P.r01 * py + P.r02 * pz + P.cx;
    const double Y = P.r10 * px + P.r11 * py + P.r12 * pz + P.cyy;
    const double Z = P.r20 * px + P.r21 * py + P.r22 * pz + P.cz;
    const double iz = 1.0 / Z;
    // jacobianRt (:354-384): row 0 = (1, 0, 0, a3, a4, a5), row 1 = (0, 1, 0, b3, b4, b5), row 2 = (0, 0, 1, 0, c4, c5)
    const double zr = py * t1 + pz * t2 - px * t3;
    const double a3 = -py * t6 + pz * t8 - px * t14, a4 = cosy * zr, a5 = py * t4 - pz * t5;
    const double b3 = pz * t4 + py * t5 + px * t15, b4 = siny * zr, b5 = -pz * t6 - py * t8;
    const double c4 = -py * t16 - pz * t17 - px * t24, c5 = py * t2 - pz * t1;
    // jacobianProy (:387-399)
    const double p00 = fx * iz, p11 = fy * iz;
    const double p02 = -(fx * X) * iz * iz, p12 = -(fy * Y) * iz * iz;
    // the two rows of the pixel through ONE accumulation, as gn_level_kernel_biobjective
#pragma unroll 1
    for (int row = 0; row < 2; row++) {
      const bool dep = row == 1;
      if (dep ? (i2 > 0 && c2) : (i == 0)) continue;
      const double ga = dep ? dgx : gx, gb = dep ? dgy : gy;
      const double gn = dep ? gain : 1.0, sub = dep ? 1.0 : 0.0;       // (x 1.0 and - 0.0 are exact: Jint as written)
      const double u = ga * p00, v = gb * p11, w = ga * p02 + gb * p12;
      const double J[6] = {gn * u, gn * v, gn * (w - sub), gn * (u * a3 + v * b3),
                           gn * (u * a4 + v * b4 + w * c4 - sub * c4), gn * (u * a5 + v * b5 + w * c5 - sub * c5)};
      add_row(acc, J, dep ? res_i2 : res_i);
    }
  }
  // contributing pixels ride through the reduction in the spare slot (lane 0 of every wave)
  acc[RED_VALID] = lane == 0 ? (double)n_contrib : 0.0;
  tile_sums(acc, lane, wave, s_red, g_part, pair, tiles);
}

// ---- finish -----------------------------------------------------------------------------------------------------------
// One workgroup per pair, k_eval_finish's body: the fixed-order sum of its slab, the system written from the upper triangle.
__global__ __launch_bounds__(ET) void k_obj_finish(const double *g_part, int tiles, phovo_pair_system *out)
{
  finish_slab<NRED>(g_part, tiles, [&](int pair, int lane, double v) { write_pair_system(out + pair, lane, v); });
}

}  // namespace

hipError_t gn_eval_objective_pairs(const GNObjectiveEvalArgs &a, int objective, int n_pairs, int *g_owner,
                                   unsigned long long *g_mask, double *g_part, phovo_pair_system *out, hipStream_t stream)
{
  if (n_pairs <= 0) return hipSuccess;
  const int tiles = gn_eval_tiles(a.n);
  const dim3 grid((unsigned)tiles, (unsigned)n_pairs);
  if (objective == PHOVO_OBJECTIVE_TRUST_REGION) {
    hipLaunchKernelGGL(k_obj_pass1_tr, grid, dim3(ET), 0, stream, a, g_owner, g_mask);
    hipLaunchKernelGGL(k_obj_pass2_tr, grid, dim3(ET), 0, stream, a, g_owner, g_mask, g_part, tiles);
  } else if (objective == PHOVO_OBJECTIVE_BIOBJECTIVE) {
    hipLaunchKernelGGL(k_obj_pass1_bi, grid, dim3(ET), 0, stream, a, g_owner, g_mask);
    hipLaunchKernelGGL(k_obj_pass2_bi, grid, dim3(ET), 0, stream, a, g_owner, g_mask, g_part, tiles);
    // (pass 2 reads entries of other tiles: the maps go back to -1 behind it, not inside it)
    const hipError_t e = fill_i32(g_owner, (size_t)n_pairs * (size_t)a.n, -1, stream);
    if (e != hipSuccess) return e;
  } else {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(k_obj_finish, dim3((unsigned)n_pairs), dim3(ET), 0, stream, g_part, tiles, out);
  return hipGetLastError();
}

}  // namespace phovo_hip
