// Trust-region (Levenberg-Marquardt) level kernel: the hot path of
//   phovo::Ceres::CPhotoconsistencyOdometryCeres::Optimize()
//   (phovo/include/CPhotoconsistencyOdometryCeres.h:433-500) with the residual ResidualRGBDPhotoconsistency (:157-269),
//   solved by Ceres's TrustRegionMinimizer with the LEVENBERG_MARQUARDT strategy -- restated here with hand-derived
//   derivatives.
//
// Residuals at state x (N = pixels of the level, indexed by TARGET pixel, zero where nothing lands): a source pixel i in
// raster order that passes the depth gate min_d < d < max_d projects to the REAL position (u, v) = ((q0 fx)/q2 + ox,
// (q1 fy)/q2 + oy), q = R(x) p + t(x); in bounds iff 0 <= v < H and 0 <= u < W; then it writes
//   r[t]   = I1(u, v) - I0[i]                                 t = W trunc(v) + trunc(u)
//   J[t,:] = GX1(u, v) du/dx + GY1(u, v) dv/dx                the exact derivative of the projection (no temp11 slip)
// where I1, GX1 and GY1 are bilinear samples (SampleLinear of third_party/sample.h, low-edge extrapolation included).
// A later pixel landing on the same t overwrites both, so the row of t belongs to owner[t] = the largest source index
// landing there: the analytic kernels' owner map.  One EVALUATION gives cost = 1/2 sum r^2, g = J^T r, H = J^T J and the
// number of owned targets.
//
// Form: persistent, one workgroup per pair at a time, one launch per level, pairs drawn from the per-XCD queues
// (draw_pair); every evaluation of a level runs inside the workgroup:
//   pass 1  warp every source pixel, atomicMax into the tagged owner map (LDS where it fits, else HBM), one in-bounds
//           ballot per 64-pixel chunk into LDS;
//   pass 2  every in-bounds pixel that owns its target: the 4 taps of I1, GX1, GY1, the row, 21 + 6 sums, r^2 and the
//           row count in registers; the analytic kernels' butterfly and fixed-order cross-wave sum;
//   serial  wave 0 runs the Levenberg-Marquardt loop in fp64 (tr_serial) on the state kept in LDS and either stops the
//           level or writes the pose constants of the next candidate.
// Every LM step costs ONE evaluation: a candidate's pass yields its cost AND its H and g; they become the next system
// when the step is accepted and are dropped otherwise.  The parameter test does not need the candidate's cost and runs
// before its pass (which it then skips).  Summation orders depend on the level size only: a pair's result is the same
// bit for bit whatever its batch or its position in it.
#include <hip/hip_runtime.h>

// The warp is computed exactly as written, without contracting products into FMAs: the CPU checker
// (tests/trust_region_ref.py) then reproduces the warped positions, and with them the truncations and bounds tests,
// bit for bit.  (Only this translation unit; the sums use explicit fma().)
#pragma clang fp contract(off)

#include "gn_device.hpp"
#include "gn_trust_region_device.hpp"      // warp_pixel, linear_axis, bilinear: shared with the evaluation kernels
#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

// Trust-region state in LDS (doubles), written by lane 0 of wave 0 only
enum {
  TR_X = 0,            // [6] the current point x
  TR_CAND = 6,         // [6] the candidate under evaluation
  TR_S = 12,           // [6] Jacobi scaling 1 / (1 + sqrt(H_jj)), from the level's first system
  TR_H = 18,           // [21] H = J^T J at x (upper triangle, row-major)
  TR_G = 39,           // [6] g = J^T r at x
  TR_COST = 45,        // cost at x
  TR_RADIUS = 46,
  TR_DECREASE = 47,
  TR_MCC = 48,         // model cost change of the candidate's step
  TR_INIT_COST = 49,
  TR_COUNT = 50
};
// Trust-region counters in LDS (ints)
enum { TRI_STEPS = 0, TRI_ACCEPTED = 1, TRI_TERM = 2, TRI_ROWS = 3, TRI_OK = 4, TRI_PHASE = 5, TRI_COUNT = 8 };

constexpr int RED_COST = 28;        // slot behind the row count: sum of r^2

__host__ __device__ constexpr size_t tr_lds_fixed_bytes(int threads)
{
  return lds_fixed_bytes(threads) + sizeof(double) * TR_COUNT + sizeof(int) * TRI_COUNT;
}

// The serial section: wave 0, every lane with the same values, lane 0 writes.  Called behind the barrier that follows the
// reduction of an evaluation (at x when the phase is 0, at the candidate when it is 1).  Returns through LDS: s_ctl[CTL_DONE]
// and, when the level goes on, the pose constants of the next candidate in s_cst.  The evaluation's sums stay spread over
// the lanes (lane j holds sum j) and reach LDS only when they become the system at x: the section keeps one 6x6 triangle
// in registers at a time.
template <int NROWS>
__device__ __forceinline__ void tr_serial(int lane, const double *s_red, double *s_tr, int *s_tri, double *s_cst, int *s_ctl,
                                          const GNTrustRegionArgs &T)
{
  // the evaluation: fixed-order sum of the wave rows (as sum_rows_solve_update)
  double v = 0.0;
  {
    const int j = lane & (NRED - 1);
    const int w0 = (lane >> 5) * (NROWS / 2);
#pragma unroll
    for (int w2 = 0; w2 < NROWS / 2; w2++) v += s_red[(w0 + w2) * NRED + j];
    v += __shfl_xor(v, 32, WAVE);
  }
  const int rows_e = (int)__shfl(v, RED_VALID, WAVE);
  const double cost_e = 0.5 * __shfl(v, RED_COST, WAVE);
  const bool sys_finite = __builtin_amdgcn_ballot_w64(lane < 27 && !finite_f64(v)) == 0;     // H and g

  const double DBL_MAX_ = 1.79769313486231570815e308;
  const int phase = s_tri[TRI_PHASE];
  double cost = s_tr[TR_COST], radius = s_tr[TR_RADIUS], decrease = s_tr[TR_DECREASE];
  int steps = s_tri[TRI_STEPS], accepted = s_tri[TRI_ACCEPTED], rows = s_tri[TRI_ROWS], ok = s_tri[TRI_OK];
  int term = -1;                  // PHOVO_TR_* once the level stops
  bool take_system = false;       // the evaluation's H and g become the system at x
  bool take_cand = false;         // the candidate becomes x

  if (phase == 0) {                                                  // iteration 0
    if (lane == 0) s_tr[TR_INIT_COST] = cost_e;
    cost = cost_e; rows = rows_e;
    if (!(finite_f64(cost_e) && sys_finite)) {
      term = PHOVO_TR_EVALUATION_FAILED;
    } else {
      radius = T.initial_radius; decrease = 2.0; ok = 1;
      take_system = true;
    }
  } else {                                                           // the candidate's evaluation
    const double cand_cost = finite_f64(cost_e) ? cost_e : DBL_MAX_;
    const double dc = cost - cand_cost;
    if (fabs(dc) <= T.function_tolerance * cost) {
      term = PHOVO_TR_FUNCTION;
    } else {
      const double mcc = s_tr[TR_MCC];
      const double rho = cand_cost == DBL_MAX_ ? -DBL_MAX_ : dc / mcc;
      if (rho > T.min_relative_decrease) {                           // accepted
        take_cand = true;
        cost = cand_cost; rows = rows_e; accepted++;
        if (!sys_finite) {
          term = PHOVO_TR_EVALUATION_FAILED;
        } else {
          take_system = true;
          const double e = 2.0 * rho - 1.0;
          radius = fmin(T.max_radius, radius / fmax(1.0 / 3.0, 1.0 - e * e * e));
          decrease = 2.0; ok = 1;
        }
      } else {
        radius = radius / decrease; decrease = decrease * 2.0; ok = 0;
      }
    }
  }
  // the new system and point to LDS (lanes 0..26 hold H and g, contiguous at TR_H)
  if (take_system && lane < 27) s_tr[TR_H + lane] = v;
  if (take_cand && lane < 6) s_tr[TR_X + lane] = s_tr[TR_CAND + lane];
  // (the shuffle runs with every lane active: a lane reads H_jj from lane tri(j, j), which a branch on lane < 6 would have
  // switched off)
  const int jd = lane < 6 ? lane : 5;
  const double hjj = __shfl(v, tri(jd, jd), WAVE);
  if (phase == 0 && take_system && lane < 6) s_tr[TR_S + lane] = 1.0 / (1.0 + sqrt(hjj));
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();

  double cand[6] = {0, 0, 0, 0, 0, 0}, mcc = 0.0;
  if (term < 0) {                                                    // the loop head
    double x[6], S[6], gs[6];
    double gmax = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      x[i] = s_tr[TR_X + i]; S[i] = s_tr[TR_S + i];
      const double g = s_tr[TR_G + i];
      gmax = fmax(gmax, fabs(x[i] - (x[i] - g)));                    // x - Plus(x, -g), formed literally
      gs[i] = S[i] * g;
    }
    if (steps >= T.max_iterations) term = PHOVO_TR_MAX_ITERATIONS;
    else if (ok && gmax <= T.gradient_tolerance) term = PHOVO_TR_GRADIENT;
    else if (radius <= T.min_radius) term = PHOVO_TR_MIN_RADIUS;
    else {
      steps++;
      // (Hs + clamp(diag Hs, 1e-6, 1e32) / radius) y = gs,  Hs = S H S
      double A[21], y[6];
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++) A[tri(a, b)] = S[a] * s_tr[TR_H + tri(a, b)] * S[b];
        const double h = A[tri(a, a)];
        A[tri(a, a)] = h + fmin(fmax(h, 1e-6), 1e32) / radius;     // min_lm_diagonal, max_lm_diagonal
      }
      const bool solved = solve6_cholesky(A, gs, y);
      double step[6];
      bool step_finite = true;
#pragma unroll
      for (int a = 0; a < 6; a++) { step[a] = -y[a]; step_finite = step_finite && finite_f64(step[a]); }
      // model cost change -(gs . step + 1/2 step^T Hs step)
      double lin = 0.0, quad = 0.0;
#pragma unroll
      for (int a = 0; a < 6; a++) {
        lin = fma(gs[a], step[a], lin);
        double hrow = 0.0;
#pragma unroll
        for (int b = 0; b < 6; b++)
          hrow = fma(S[a] * s_tr[TR_H + (a <= b ? tri(a, b) : tri(b, a))] * S[b], step[b], hrow);
        quad = fma(step[a], hrow, quad);
      }
      mcc = -(lin + 0.5 * quad);
      if (!solved || !step_finite || !(mcc > 0.0)) {
        term = PHOVO_TR_INVALID_STEP;
      } else {
        double dn2 = 0.0, xn2 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
          cand[a] = x[a] + S[a] * step[a];
          const double dd = x[a] - cand[a];
          dn2 = fma(dd, dd, dn2);
          xn2 = fma(x[a], x[a], xn2);
        }
        if (sqrt(dn2) <= T.parameter_tolerance * (sqrt(xn2) + T.parameter_tolerance)) term = PHOVO_TR_PARAMETER;
      }
    }
  }
  if (term < 0) write_pose_constants(cand[0], cand[1], cand[2], cand[3], cand[4], cand[5], s_cst, lane);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; i++) s_tr[TR_CAND + i] = cand[i];
    s_tr[TR_COST] = cost; s_tr[TR_RADIUS] = radius; s_tr[TR_DECREASE] = decrease; s_tr[TR_MCC] = mcc;
    s_tri[TRI_STEPS] = steps; s_tri[TRI_ACCEPTED] = accepted; s_tri[TRI_ROWS] = rows; s_tri[TRI_OK] = ok;
    s_tri[TRI_PHASE] = 1;
    s_tri[TRI_TERM] = term;
    s_ctl[CTL_DONE] = term >= 0 ? 1 : 0;
  }
}

// T threads per workgroup.  OWNER_LDS: owner map in LDS (else in HBM, args.lv.g_owner + pair * n).
template <int T, bool OWNER_LDS>
__global__ __launch_bounds__(T, 2) void gn_level_kernel_trust_region(const GNTrustRegionArgs B)
{
  constexpr int NW = T / WAVE;
  const GNLevelArgs &A = B.lv;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *s_cst = reinterpret_cast<double *>(lds_raw);                 // [32]
  double *s_state = s_cst + 32;                                        // [8] (unused: the state lives in s_tr)
  double *s_red = s_state + 8;                                         // [NW][NRED]
  int *s_ctl = reinterpret_cast<int *>(s_red + NW * NRED);             // [CTL_COUNT]
  double *s_tr = reinterpret_cast<double *>(s_ctl + CTL_COUNT);        // [TR_COUNT]
  int *s_tri = reinterpret_cast<int *>(s_tr + TR_COUNT);               // [TRI_COUNT]
  unsigned long long *s_mask = reinterpret_cast<unsigned long long *>(s_tri + TRI_COUNT);    // [n_chunks] in bounds
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
  // (in HBM: one map per resident workgroup, wiped per pair -- the grid never exceeds the resident slots)
  int *owner = OWNER_LDS ? s_owner : A.g_owner + (size_t)blockIdx.x * (size_t)n;

  for (int k = tid; k < n; k += T) owner[k] = -1;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wave == 0) {
    double st[6];
#pragma unroll
    for (int j = 0; j < 6; j++) st[j] = A.states[(size_t)pair * 6 + j];
    write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, lane);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 6; j++) s_tr[TR_X + j] = st[j];
#pragma unroll
      for (int j = 0; j < TRI_COUNT; j++) s_tri[j] = 0;
#pragma unroll
      for (int j = 0; j < 6; j++) s_tr[TR_S + j] = 0.0;          // (stays 0 when the first evaluation fails)
      s_ctl[CTL_DONE] = 0;
    }
  }
  lds_barrier();

  const RowColFromIndex rc = make_rowcol_from_index(W);
  int evaluation = 0;
  while (true) {
    // the point of this evaluation: Rt of eigenPose (the constants write_pose_constants stores)
    const double R[9] = {uniform_f64(s_cst[C_T15]), uniform_f64(s_cst[C_R01]), uniform_f64(s_cst[C_R02]),
                         uniform_f64(s_cst[C_T14]), uniform_f64(s_cst[C_R11]), uniform_f64(s_cst[C_R12]),
                         -uniform_f64(s_cst[C_T3]), uniform_f64(s_cst[C_T1]), uniform_f64(s_cst[C_T2])};
    const double tv[3] = {uniform_f64(s_cst[C_X]), uniform_f64(s_cst[C_Y]), uniform_f64(s_cst[C_Z])};

    // tags of this evaluation (1..OWNER_TAG_PERIOD); when they start over the map is wiped
    const int tg = evaluation % OWNER_TAG_PERIOD + 1;
    if (evaluation > 0 && tg == 1) {                                    // uniform: every wave takes it
      for (int k = tid; k < n; k += T) owner[k] = -1;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();
    }
    const int owner_tag = tg << OWNER_TAG_SHIFT;

    // ---- pass 1: warp, in-bounds ballot, owner map (last raster writer wins: largest source index) ----------------
    for (int chunk = wave; chunk < A.n_chunks; chunk += NW) {
      const int i = chunk * WAVE + lane;
      const double d = i < n ? plane_load<double>(rS, i, oD) : 0.0;
      const Warp w = warp_pixel((double)i, d, rc, A, R, tv);
      const bool ok = i < n && w.ok;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
      if (lane == 0) s_mask[chunk] = m;
      if (ok) atomicMax(&owner[W * (int)w.v + (int)w.u], owner_tag | i);                    // :255-257
    }
    if (!OWNER_LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (atomics without return: settled before the barrier)
    lds_barrier();

    // ---- pass 2: the row of every owned target, its residual, the normal equations --------------------------------
    const double cy = uniform_f64(s_cst[C_CY]), sy = uniform_f64(s_cst[C_SY]);
    const double cp = uniform_f64(s_cst[C_T24]);
    const double sp_sr = uniform_f64(s_cst[C_T16]), sp_cr = uniform_f64(s_cst[C_T17]);
    const double sr_cp = R[7], cr_cp = R[8];
    double acc[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = 0.0;
    for (int chunk = wave; chunk < A.n_chunks; chunk += NW) {
      const unsigned long long mbits = s_mask[chunk];
      if (!((mbits >> lane) & 1ull)) continue;
      const int i = chunk * WAVE + lane;
      const double d = plane_load<double>(rS, i, oD);
      const Warp w = warp_pixel((double)i, d, rc, A, R, tv);
      const int t = W * (int)w.v + (int)w.u;
      const int raw = OWNER_LDS ? owner[t] : __hip_atomic_load(&owner[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (raw != (owner_tag | i)) continue;                          // a later pixel overwrote this target
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
      // d(u, v)/dx: u = fx q0 / q2 + ox, q = R(yaw, pitch, roll) p + t
      const double iz = 1.0 / w.q2;
      const double du0 = A.fx * iz, dv1 = A.fy * iz;                   // du/dq0, dv/dq1
      const double du2 = -A.fx * w.q0 * iz * iz, dv2 = -A.fy * w.q1 * iz * iz;    // du/dq2, dv/dq2
      const double ju = gxs * du0, jv = gys * dv1, jw = gxs * du2 + gys * dv2;
      // dq/dyaw = (-a1, a0, 0); dq/dpitch = (cy a2, sy a2, -(cp px + sp (sr py + cr pz))); dq/droll = R[:,2] py - R[:,1] pz
      const double dq2_pitch = -(cp * w.px + sp_sr * w.py + sp_cr * w.pz);
      const double dq0_roll = R[2] * w.py - R[1] * w.pz;
      const double dq1_roll = R[5] * w.py - R[4] * w.pz;
      const double dq2_roll = cr_cp * w.py - sr_cp * w.pz;
      const double J[6] = {ju, jv, jw, jv * w.a0 - ju * w.a1, (ju * cy + jv * sy) * w.a2 + jw * dq2_pitch,
                           ju * dq0_roll + jv * dq1_roll + jw * dq2_roll};
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++) {
          acc[q] = fma(J[a], J[b], acc[q]);
          q++;
        }
      }
#pragma unroll
      for (int a = 0; a < 6; a++) acc[21 + a] = fma(J[a], res, acc[21 + a]);
      acc[RED_VALID] += 1.0;
      acc[RED_COST] = fma(res, res, acc[RED_COST]);
    }
    reduce_wave_to_row(acc, lane, wave, s_red);
    lds_barrier();
    if (wave == 0) tr_serial<NW>(lane, s_red, s_tr, s_tri, s_cst, s_ctl, B);
    lds_barrier();
    evaluation++;
    if (s_ctl[CTL_DONE]) break;
  }

  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 6; j++) A.states[(size_t)pair * 6 + j] = s_tr[TR_X + j];
    const int L = A.level;
    const int term = s_tri[TRI_TERM];
    if (B.tr_reports) {
      phovo_trust_region_level &r = B.tr_reports[pair].level[L];
      r.steps = s_tri[TRI_STEPS];
      r.accepted = s_tri[TRI_ACCEPTED];
      r.termination = term;
      r.rows = s_tri[TRI_ROWS];
      r.initial_cost = s_tr[TR_INIT_COST];
      r.final_cost = s_tr[TR_COST];
      r.final_radius = s_tr[TR_RADIUS];
#pragma unroll
      for (int j = 0; j < 6; j++) r.jacobi_scaling[j] = s_tr[TR_S + j];
    }
    if (A.reports) {
      A.reports[pair].iterations[L] = s_tri[TRI_STEPS];
      A.reports[pair].valid_pixels[L] = s_tri[TRI_ROWS];
      double gn2 = 0.0;
#pragma unroll
      for (int j = 0; j < 6; j++) gn2 = fma(s_tr[TR_G + j], s_tr[TR_G + j], gn2);
      A.reports[pair].gradient_norm = term == PHOVO_TR_EVALUATION_FAILED ? __builtin_nan("") : sqrt(gn2);
      // NONFINITE: an evaluation was not finite, or the state is (a NaN / inf initial state: no pixel warps, the system
      // is finite and zero, and the level ends without a step)
      bool x_finite = true;
#pragma unroll
      for (int j = 0; j < 6; j++) x_finite = x_finite && finite_f64(s_tr[TR_X + j]);
      uint32_t new_flags = 0;
      if (term == PHOVO_TR_EVALUATION_FAILED || !x_finite) new_flags |= PHOVO_PAIR_NONFINITE;
      if (s_tri[TRI_ROWS] < 6) new_flags |= PHOVO_PAIR_RANK_DEFICIENT;
      if (new_flags) atomicOr(&A.reports[pair].flags, new_flags);
    }
    s_ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

// Instantiations (two waves per SIMD: 256 registers):
//   SMALL  256 threads, two workgroups per CU, owner map in LDS (levels whose map takes at most half of it)
//   LARGE  512 threads, one workgroup per CU, owner map in LDS
//   HBM    512 threads, one workgroup per CU, owner map in HBM (lv.g_owner: [workgroups][n]), ballots in LDS
#define PHOVO_KERNEL_TR_SMALL gn_level_kernel_trust_region<256, true>
#define PHOVO_KERNEL_TR_LARGE gn_level_kernel_trust_region<512, true>
#define PHOVO_KERNEL_TR_HBM   gn_level_kernel_trust_region<512, false>

}  // namespace

bool gn_plan_level_trust_region(int n, GNLaunchPlan *plan)
{
  const size_t n_chunks = (size_t)(n + WAVE - 1) / WAVE;
  const size_t mask = sizeof(unsigned long long) * n_chunks;
  const size_t owner = sizeof(int) * (size_t)n;
  plan->variant = 0; plan->source_in_lds = false; plan->owner_lds_entries = 0; plan->mask_in_hbm = false;
  plan->depth_lds_chunks = 0;
  if (tr_lds_fixed_bytes(256) + mask + owner <= LDS_LIMIT / 2) {
    plan->threads = 256; plan->wgs_per_cu = 2; plan->owner_in_lds = true;
    plan->lds_bytes = (int)(tr_lds_fixed_bytes(256) + mask + owner);
    return true;
  }
  if (tr_lds_fixed_bytes(512) + mask + owner <= LDS_LIMIT) {
    plan->threads = 512; plan->wgs_per_cu = 1; plan->owner_in_lds = true;
    plan->lds_bytes = (int)(tr_lds_fixed_bytes(512) + mask + owner);
    return true;
  }
  if (n > OWNER_INDEX_MASK || tr_lds_fixed_bytes(512) + mask > LDS_LIMIT) return false;
  plan->threads = 512; plan->wgs_per_cu = 1; plan->owner_in_lds = false;
  plan->lds_bytes = (int)(tr_lds_fixed_bytes(512) + mask);
  return true;
}

hipError_t gn_prepare_trust_region_kernels()
{
  hipError_t e;
  for (const void *k : {reinterpret_cast<const void *>(&PHOVO_KERNEL_TR_SMALL), reinterpret_cast<const void *>(&PHOVO_KERNEL_TR_LARGE),
                        reinterpret_cast<const void *>(&PHOVO_KERNEL_TR_HBM)})
    if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT)) != hipSuccess) return e;
  return hipSuccess;
}

hipError_t gn_launch_level_trust_region(const GNTrustRegionArgs &b, const GNLaunchPlan &plan, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  if (!plan.owner_in_lds && !b.lv.g_owner) return hipErrorInvalidValue;
  const auto kernel = !plan.owner_in_lds ? PHOVO_KERNEL_TR_HBM : (plan.threads == 256 ? PHOVO_KERNEL_TR_SMALL : PHOVO_KERNEL_TR_LARGE);
  return launch_persistent(kernel, b.lv.n_pairs, cu_count, plan.wgs_per_cu, plan.threads, (size_t)plan.lds_bytes, stream, b);
}

}  // namespace phovo_hip
