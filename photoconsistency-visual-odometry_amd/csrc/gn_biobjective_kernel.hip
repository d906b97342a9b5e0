// Bi-objective Gauss-Newton level kernel: the hot path of
//   phovo::Analytic::CPhotoconsistencyOdometryBiObjective::Optimize()
//   (phovo/include/CPhotoconsistencyOdometryBiObjective.h:587-648) with ComputeResidualsAndJacobians (:242-450), which
//   minimises the photometric and the depth error together.
//
// What the reference does per iteration (N = pixels of the level): a source pixel i that passes the depth gate and whose
// rounded warp t lands in bounds -- a CONTRIBUTING pixel -- writes, in raster order and in this order,
//   J[i]  = Jint(i) = grad I1(i) . Jproj . JRt                    (:432-437; the true chain rule, no temp11 slip)
//   r[t]  = I1[t] - I0[i]                                         (:440)
//   J[2i] = Jdep(i) = gain * (grad D1(i) . Jproj . JRt - JRt[z,:])  (:443-448)
//   r[2t] = gain * (D1[t] - D0[i])                                (:451-452)
// into a zeroed 2N-row system, and the step is the analytic one over those 2N rows (:637-639).  Rows collide: the depth
// write of pixel i to row 2i (residual 2t) lands on a row an intensity write also uses, and the last writer wins.  With
// owner[t] = the largest contributing source index that lands on t (the analytic path's owner map):
//   J of row m: Jint(m) if m < N, m > 0 and pixel m contributes; else Jdep(m/2) if m is even and pixel m/2 contributes;
//               else 0 (at m = 0 pixel 0 writes its depth row after its intensity row: depth wins);
//   r of row m: the larger of the intensity candidate owner[m] (m < N) and the depth candidate owner[m/2] (m even) wins,
//               a tie (m = 0 only) goes to depth, no candidate: 0.
// So a contributing pixel i OWNS row i (unless i = 0) with Jint(i), and row 2i (unless 0 < 2i < N and pixel 2i
// contributes) with Jdep(i); every owned row adds its outer product to H and its Jacobian times its resolved residual to g.
//
// Form: persistent, one workgroup per pair at a time, every iteration of a level inside the workgroup (one launch per
// level), pairs drawn from the per-XCD queues of the analytic kernels (draw_pair).
//   pass 1  warp every source pixel (depth gate, C round(), bounds), atomicMax into the owner map, one ballot per
//           64-pixel chunk of "contributes" into LDS;
//   pass 2  every contributing pixel: Jint and Jdep, the two rows it owns, the residuals resolved from owner[i],
//           owner[i/2], owner[2i] and the ballot of pixel 2i, 21 + 6 sums in registers;
//   reduce  the analytic kernels' transposed butterfly and fixed-order cross-wave sum, LDL^T solve on wave 0.
// Owner-map entries carry an iteration tag (OWNER_TAG_SHIFT, as the analytic kernel's map in HBM) so that pass 2 only
// reads the map and nothing has to be reset between iterations; it is wiped once per pair.  The map lives in LDS where it
// fits (every active level of the shipped 4-, 5- and 6-level files at 640x480) and in HBM otherwise (640x480 level 0).
#include <hip/hip_runtime.h>

#include "gn_device.hpp"
#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

// T threads per workgroup.  OWNER_LDS: owner map in LDS (else in HBM, args.lv.g_owner + pair * n).
template <int T, bool OWNER_LDS>
__global__ __launch_bounds__(T, 2) void gn_level_kernel_biobjective(const GNBiObjectiveArgs B)
{
  constexpr int NW = T / WAVE;
  const GNLevelArgs &A = B.lv;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *s_cst = reinterpret_cast<double *>(lds_raw);                 // [32]
  double *s_state = s_cst + 32;                                        // [8]
  double *s_red = s_state + 8;                                         // [NW][NRED]
  int *s_ctl = reinterpret_cast<int *>(s_red + NW * NRED);             // [CTL_COUNT]
  unsigned long long *s_mask = reinterpret_cast<unsigned long long *>(s_ctl + CTL_COUNT);    // [n_chunks] contributes
  int *s_owner = reinterpret_cast<int *>(s_mask + A.n_chunks);         // [n] (OWNER_LDS)

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  if (tid == 0) s_ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  for (;;) {                                // work queue, as in gn_level_kernel
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // see gn_level_kernel
  __syncthreads();
  const int pair = __builtin_amdgcn_readfirstlane(s_ctl[CTL_PAIR]);
  if (pair >= A.n_pairs) break;
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(src_frame, A.frame_bytes), rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int oI = (int)A.plane_off[PLANE_I], oD = (int)A.plane_off[PLANE_D];
  const int oGX = (int)A.plane_off[PLANE_GX], oGY = (int)A.plane_off[PLANE_GY];
  const int oDGX = (int)B.dgx_off, oDGY = (int)B.dgy_off;
  int *owner = OWNER_LDS ? s_owner : A.g_owner + (size_t)pair * (size_t)n;
  // gain = mean(target gray) / mean(target depth) (:300), computed once per target frame and level at upload
  const double gain = uniform_f64(*reinterpret_cast<const double *>(tgt_frame + B.gain_off));

  for (int k = tid; k < n; k += T) owner[k] = -1;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wave == 0) {
    double st[6];
#pragma unroll
    for (int j = 0; j < 6; j++) st[j] = A.states[(size_t)pair * 6 + j];
    write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, lane);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 6; j++) s_state[j] = st[j];
      s_ctl[CTL_DONE] = 0;
      s_ctl[CTL_FLAGS] = 0;
    }
  }
  lds_barrier();

  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const double min_d = A.min_depth, max_d = A.max_depth;
  const RowColFromIndex rc = make_rowcol_from_index(W);
  int iteration = 0, last_valid = 0;
  double last_gnorm = 0.0;
  while (true) {
    const double cx = uniform_f64(s_cst[C_X]), cyy = uniform_f64(s_cst[C_Y]), cz = uniform_f64(s_cst[C_Z]);
    const double r00 = uniform_f64(s_cst[C_T15]), r01 = uniform_f64(s_cst[C_R01]), r02 = uniform_f64(s_cst[C_R02]);
    const double r10 = uniform_f64(s_cst[C_T14]), r11 = uniform_f64(s_cst[C_R11]), r12 = uniform_f64(s_cst[C_R12]);
    const double t1 = uniform_f64(s_cst[C_T1]), t2 = uniform_f64(s_cst[C_T2]), t3 = uniform_f64(s_cst[C_T3]);
    // Rt (:275-291): row 2 is (-sin(pitch), temp1, temp2)
    const double r20 = -t3, r21 = t1, r22 = t2;

    // tags of this iteration (1..OWNER_TAG_PERIOD); when they start over the map is wiped
    const int tg = iteration % OWNER_TAG_PERIOD + 1;
    if (iteration > 0 && tg == 1) {                                     // uniform: every wave takes it
      for (int k = tid; k < n; k += T) owner[k] = -1;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
    }
    const int owner_tag = tg << OWNER_TAG_SHIFT;

    // ---- pass 1: warp, contributes-ballot, owner map (last raster writer wins: largest source index) ------------
    for (int chunk = wave; chunk < A.n_chunks; chunk += NW) {
      const int i = chunk * WAVE + lane;
      const double pz = i < n ? plane_load<double>(rS, i, oD) : 0.0;                 // :310
      double cd, rd;
      rowcol_from_index((double)i, rc, cd, rd);                                       // (exact: gn_device.hpp)
      const double px = (cd - ox) * pz * ifx;                                         // :313
      const double py = (rd - oy) * pz * ify;                                         // :314
      const double X = r00 * px + r01 * py + r02 * pz + cx;                           // :322
      const double Y = r10 * px + r11 * py + r12 * pz + cyy;
      const double Z = r20 * px + r21 * py + r22 * pz + cz;
      const double iz = 1.0 / Z;                                                      // :325
      const double tc = (X * fx) * iz + ox;                                           // :326
      const double tr = (Y * fy) * iz + oy;                                           // :327
      // C round() (:328-329) for arguments > -0.5 (round_half_up_from), then the bounds (:333-334); NaN fails `> -0.5`
      const bool ok = i < n && min_d < pz && pz < max_d && tr > -0.5 && tc > -0.5 &&
                      round_half_up_from(tr) < (double)H && round_half_up_from(tc) < (double)W;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
      if (lane == 0) s_mask[chunk] = m;
      if (ok) {
        const int t = (int)round_half_up_from(tr) * W + (int)round_half_up_from(tc);
        atomicMax(&owner[t], owner_tag | i);
      }
    }
    if (!OWNER_LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (atomics without return: settled before the barrier)
    lds_barrier();

    // ---- pass 2: the rows a contributing pixel owns, their resolved residuals, the normal equations ------------
    const double t4 = uniform_f64(s_cst[C_T4]), t5 = uniform_f64(s_cst[C_T5]), t6 = uniform_f64(s_cst[C_T6]);
    const double t8 = uniform_f64(s_cst[C_T8]), t14 = r10, t15 = r00;
    const double t16 = uniform_f64(s_cst[C_T16]), t17 = uniform_f64(s_cst[C_T17]), t24 = uniform_f64(s_cst[C_T24]);
    const double cosy = uniform_f64(s_cst[C_CY]), siny = uniform_f64(s_cst[C_SY]);

    double acc[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = 0.0;
    int n_contrib = 0;
    auto owner_at = [&](int k) {          // the entry of this iteration at k, or -1
      const int raw = OWNER_LDS ? owner[k] : __hip_atomic_load(&owner[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return (raw & ~OWNER_INDEX_MASK) == owner_tag ? (raw & OWNER_INDEX_MASK) : -1;
    };
    auto add_row = [&](const double (&J)[6], const double res) {
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++) {
          acc[q] = fma(J[a], J[b], acc[q]);                                           // J^T J  :639
          q++;
        }
      }
#pragma unroll
      for (int a = 0; a < 6; a++) acc[21 + a] = fma(J[a], res, acc[21 + a]);          // J^T r  :637
    };
    for (int chunk = wave; chunk < A.n_chunks; chunk += NW) {
      const unsigned long long mbits = s_mask[chunk];
      if (lane == 0) n_contrib += __builtin_popcountll(mbits);
      if (!((mbits >> lane) & 1ull)) continue;
      const int i = chunk * WAVE + lane;
      const double pz = plane_load<double>(rS, i, oD);
      const double gx = plane_load<double>(rT, i, oGX), gy = plane_load<double>(rT, i, oGY);     // at the SOURCE index  :424-425
      const double dgx = plane_load<double>(rT, i, oDGX), dgy = plane_load<double>(rT, i, oDGY); // :430-431
      double cd, rd;
      rowcol_from_index((double)i, rc, cd, rd);
      const double px = (cd - ox) * pz * ifx;
      const double py = (rd - oy) * pz * ify;
      const double X = r00 * px + r01 * py + r02 * pz + cx;
      const double Y = r10 * px + r11 * py + r12 * pz + cyy;
      const double Z = r20 * px + r21 * py + r22 * pz + cz;
      const double iz = 1.0 / Z;
      // jacobianRt (:354-384): row 0 = (1, 0, 0, a3, a4, a5), row 1 = (0, 1, 0, b3, b4, b5), row 2 = (0, 0, 1, 0, c4, c5)
      const double zr = py * t1 + pz * t2 - px * t3;
      const double a3 = -py * t6 + pz * t8 - px * t14, a4 = cosy * zr, a5 = py * t4 - pz * t5;
      const double b3 = pz * t4 + py * t5 + px * t15, b4 = siny * zr, b5 = -pz * t6 - py * t8;
      const double c4 = -py * t16 - pz * t17 - px * t24, c5 = py * t2 - pz * t1;
      // jacobianProy (:387-399)
      const double p00 = fx * iz, p11 = fy * iz;
      const double p02 = -(fx * X) * iz * iz, p12 = -(fy * Y) * iz * iz;
      // pixel 2i contributes?  (only asked for 0 < 2i < N)
      const int i2 = 2 * i;
      const bool c2 = i2 < n && ((s_mask[i2 >> 6] >> (i2 & 63)) & 1ull);
      const int o_i = owner_at(i);
      const int o_half = owner_at(i >> 1);
      // The two rows of the pixel, one after the other through ONE accumulation (a loop, not unrolled: one copy of the
      // 27 FMAs instead of two keeps the live registers down; the kernel is compiled for two waves per SIMD, 172 VGPRs).
      //   row i (i > 0): Jint(i); residual: intensity candidate owner[i] vs depth candidate owner[i/2] (i even)
      //   row 2i unless 0 < 2i < N and pixel 2i contributes: Jdep(i); residual: intensity candidate owner[2i] (2i < N)
      //   vs depth candidate owner[i]
#pragma unroll 1
      for (int row = 0; row < 2; row++) {
        const bool dep = row == 1;
        if (dep ? (i2 > 0 && c2) : (i == 0)) continue;
        const double ga = dep ? dgx : gx, gb = dep ? dgy : gy;
        const double gn = dep ? gain : 1.0, sub = dep ? 1.0 : 0.0;       // (x 1.0 and - 0.0 are exact: Jint as written)
        const double u = ga * p00, v = gb * p11, w = ga * p02 + gb * p12;
        const double J[6] = {gn * u, gn * v, gn * (w - sub), gn * (u * a3 + v * b3),
                             gn * (u * a4 + v * b4 + w * c4 - sub * c4), gn * (u * a5 + v * b5 + w * c5 - sub * c5)};
        // candidates: intensity writer of the row (its target is the row), depth writer (its target is half the row)
        const int o_int = dep ? (i2 < n ? owner_at(i2) : -1) : o_i;
        const int o_dep = dep ? o_i : ((i & 1) ? -1 : o_half);
        const int row_m = dep ? i2 : i;
        double res = 0.0;
        if (o_dep >= 0 && o_dep >= o_int) res = gain * (plane_load<double>(rT, row_m >> 1, oD) - plane_load<double>(rS, o_dep, oD));
        else if (o_int >= 0) res = plane_load<double>(rT, row_m, oI) - plane_load<double>(rS, o_int, oI);
        add_row(J, res);
      }
    }
    // contributing pixels ride through the reduction in the spare slot (lane 0 of every wave)
    acc[RED_VALID] = lane == 0 ? (double)n_contrib : 0.0;
    reduce_wave_to_row(acc, lane, wave, s_red);
    lds_barrier();
    if (wave == 0)
      sum_rows_solve_update<NW>(lane, s_red, s_state, s_cst, s_ctl, A.lambda, A.max_iter, A.min_grad_norm, iteration,
                                last_gnorm, last_valid);
    lds_barrier();
    iteration++;
    if (s_ctl[CTL_DONE]) break;
  }

  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 6; j++) A.states[(size_t)pair * 6 + j] = s_state[j];
    if (A.reports) {
      A.reports[pair].iterations[A.level] = iteration;
      A.reports[pair].gradient_norm = last_gnorm;
      A.reports[pair].valid_pixels[A.level] = last_valid;
      const uint32_t new_flags = (uint32_t)s_ctl[CTL_FLAGS];
      if (new_flags) atomicOr(&A.reports[pair].flags, new_flags);
    }
    s_ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

// Instantiations (two waves per SIMD: 256 registers, no spills in the pixel loops):
//   SMALL  256 threads, two workgroups per CU, owner map in LDS (levels whose map takes at most half of it)
//   LARGE  512 threads, one workgroup per CU, owner map in LDS
//   HBM    512 threads, one workgroup per CU, owner map in HBM, ballots in LDS
#define PHOVO_KERNEL_BI_SMALL gn_level_kernel_biobjective<256, true>
#define PHOVO_KERNEL_BI_LARGE gn_level_kernel_biobjective<512, true>
#define PHOVO_KERNEL_BI_HBM   gn_level_kernel_biobjective<512, false>

}  // namespace

bool gn_plan_level_biobjective(int n, GNLaunchPlan *plan)
{
  const size_t n_chunks = (size_t)(n + WAVE - 1) / WAVE;
  const size_t mask = sizeof(unsigned long long) * n_chunks;
  const size_t owner = sizeof(int) * (size_t)n;
  plan->variant = 0; plan->source_in_lds = false; plan->owner_lds_entries = 0; plan->mask_in_hbm = false;
  plan->depth_lds_chunks = 0;
  if (lds_fixed_bytes(256) + mask + owner <= LDS_LIMIT / 2) {
    plan->threads = 256; plan->wgs_per_cu = 2; plan->owner_in_lds = true;
    plan->lds_bytes = (int)(lds_fixed_bytes(256) + mask + owner);
    return true;
  }
  if (lds_fixed_bytes(512) + mask + owner <= LDS_LIMIT) {
    plan->threads = 512; plan->wgs_per_cu = 1; plan->owner_in_lds = true;
    plan->lds_bytes = (int)(lds_fixed_bytes(512) + mask + owner);
    return true;
  }
  if (n > OWNER_INDEX_MASK || lds_fixed_bytes(512) + mask > LDS_LIMIT) return false;
  plan->threads = 512; plan->wgs_per_cu = 1; plan->owner_in_lds = false;
  plan->lds_bytes = (int)(lds_fixed_bytes(512) + mask);
  return true;
}

hipError_t gn_prepare_biobjective_kernels()
{
  hipError_t e;
  for (const void *k : {reinterpret_cast<const void *>(&PHOVO_KERNEL_BI_SMALL), reinterpret_cast<const void *>(&PHOVO_KERNEL_BI_LARGE),
                        reinterpret_cast<const void *>(&PHOVO_KERNEL_BI_HBM)})
    if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT)) != hipSuccess) return e;
  return hipSuccess;
}

hipError_t gn_launch_level_biobjective(const GNBiObjectiveArgs &b, const GNLaunchPlan &plan, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  if (!plan.owner_in_lds && !b.lv.g_owner) return hipErrorInvalidValue;
  const auto kernel = !plan.owner_in_lds ? PHOVO_KERNEL_BI_HBM : (plan.threads == 256 ? PHOVO_KERNEL_BI_SMALL : PHOVO_KERNEL_BI_LARGE);
  return launch_persistent(kernel, b.lv.n_pairs, cu_count, plan.wgs_per_cu, plan.threads, (size_t)plan.lds_bytes, stream, b);
}

}  // namespace phovo_hip
