// PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC: forward-additive alignment on intensity AND depth.  Every source
// pixel that is a row of the bilinear extension with the true warp Jacobian (gn_bilinear_kernel.hip, CORRECTED; the rows of
// gn_affine_kernel.hip at alpha = beta = 0, same warp expressions, same compile flags) contributes
//   r_I = I1(u, v) - I0                                   J_I = gx dU/dp + gy dV/dp
// and, where the four taps of the target's depth pass the depth gate (and the residual gate, if it is on), a second row
//   r_D = sigma (D1(u, v) - Z')                           J_D = sigma (dgx dU/dp + dgy dV/dp - dZ'/dp)
// with Z' the third coordinate of the moved point, D1(u, v) the bilinear sample on the SAME clamped taps and weights as I1
// and (dgx, dgy) the exact derivative of that interpolant (0 where clamping makes both taps of a difference one pixel).
// The target's depth is the depth plane a source upload of that frame left in the pool: no new planes.
// H = sum J_I J_I^T + sum J_D J_D^T, g = sum J_I r_I + sum J_D r_D: 6 x 6, the pose alone.  fp64 planes, no Huber weights.
// The form is gn_level_kernel_affine's: persistent, one 256-thread workgroup runs all iterations of a level for a pair, one
// pass per iteration, no scatter, no owner map, no atomics, any level size; sixteen 8-byte gathers per pixel (twelve taps of
// I1, GX1, GY1 and four of D1), one chunk's taps in flight.  Sums: 21 + 6, the two row counts and the two costs -- 31 slots
// of ONE block of NRED -- through the analytic kernels' butterfly and fixed-order cross-wave sum, then the 6 x 6 LDL^T solve
// and update those kernels use, so every summation order depends on the level size only.
#include <hip/hip_runtime.h>

#include "gn_device.hpp"
#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

// slots of the block behind the 21 + 6 sums and the photometric row count (RED_VALID = 27)
enum { RED_DEPTH_ROWS = 28, RED_COST_I = 29, RED_COST_D = 30 };
static_assert(RED_COST_D < NRED, "one block of NRED carries every sum");

template <int T, int WPS>
__global__ __launch_bounds__(T, WPS) void gn_level_kernel_geometric(const GNGeometricArgs B)
{
  const GNLevelArgs &A = B.lv;
  constexpr int NW = T / WAVE;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *s_cst = reinterpret_cast<double *>(lds_raw);                 // [32]
  double *s_state = s_cst + 32;                                        // [8]: the pose in the first 6
  double *s_red = s_state + 8;                                         // [NW][NRED]
  int *s_ctl = reinterpret_cast<int *>(s_red + NW * NRED);             // [CTL_COUNT]

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
  const __amdgpu_buffer_rsrc_t rI0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_I], n);
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_D], n);
  // one descriptor for the target frame; a plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];
  const int o_d = (int)A.plane_off[PLANE_D];

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
  __syncthreads();

  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const double min_d = A.min_depth, max_d = A.max_depth;
  const double sigma = B.depth_weight, gate = B.max_depth_residual;
  const bool gate_on = gate > 0.0;
  const double wlim = (double)W - 0.5, hlim = (double)H - 0.5;
  const int k0 = wave * WAVE + lane;
  const int r0 = k0 / W, c0 = k0 - r0 * W;
  const int step_r = (NW * WAVE) / W, step_c = (NW * WAVE) - step_r * W;
  const RowColStep rc_step = make_rowcol_step(step_r, step_c, W);
  const double cd0 = (double)c0, rd0 = (double)r0;

  int iteration = 0;
  double last_gnorm = 0.0, last_cost_i = 0.0, last_cost_d = 0.0;
  int last_valid = 0, last_depth_rows = 0;
  while (true) {
    const double cx = uniform_f64(s_cst[C_X]), cyy = uniform_f64(s_cst[C_Y]), cz = uniform_f64(s_cst[C_Z]);
    const double r01 = uniform_f64(s_cst[C_R01]), r02 = uniform_f64(s_cst[C_R02]);
    const double r11 = uniform_f64(s_cst[C_R11]), r12 = uniform_f64(s_cst[C_R12]);
    const double t1 = uniform_f64(s_cst[C_T1]), t2 = uniform_f64(s_cst[C_T2]), t3 = uniform_f64(s_cst[C_T3]);
    const double t4 = uniform_f64(s_cst[C_T4]), t5 = uniform_f64(s_cst[C_T5]), t6 = uniform_f64(s_cst[C_T6]);
    const double t8 = uniform_f64(s_cst[C_T8]), t14 = uniform_f64(s_cst[C_T14]), t15 = uniform_f64(s_cst[C_T15]);
    const double t16 = uniform_f64(s_cst[C_T16]), t17 = uniform_f64(s_cst[C_T17]), t24 = uniform_f64(s_cst[C_T24]);
    const double cosy = uniform_f64(s_cst[C_CY]), siny = uniform_f64(s_cst[C_SY]);
    const double t7 = -t6, t9 = -t8, t21 = -t5;

    double acc[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = 0.0;

    // The software pipeline of gn_level_kernel_affine: the geometry of chunk i+1, then the four bilinear samples of chunk i
    // (the wait for its taps), then the sixteen taps of chunk i+1 go out into the registers just freed, then the two
    // Jacobian rows and the sums of chunk i run while they travel.
    struct Warped {
      double px, py, pz, Zr, t25, ax, ay, i0;
      int idx[4];                           // the clamped taps p00, p01, p10, p11: indices into a plane
      unsigned long long m;                 // lanes that are valid and land in bounds
    };
    struct Sampled {
      double i1, gx, gy;                    // the bilinear samples of I1, GX1, GY1
      double d1, dgx, dgy;                  // the bilinear sample of D1 and the derivative of its interpolant
      bool taps_ok;                         // every D1 tap passes the depth gate
    };
    double tap[16] = {};                    // I1, GX1, GY1, D1 at p00, p01, p10, p11 of the chunk whose taps are in flight
    int k = k0;
    double cd = cd0, rd = rd0;
    double pz_next = plane_load<double>(rD0, k);                          // past the plane: 0
    double i0_next = plane_load<double>(rI0, k);
    auto warp = [&](Warped &w) {
      const double pz = pz_next;
      w.i0 = i0_next;
      pz_next = plane_load<double>(rD0, k + NW * WAVE);
      i0_next = plane_load<double>(rI0, k + NW * WAVE);
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
      k += NW * WAVE;
      rowcol_advance(cd, rd, rc_step);
    };
    auto issue = [&](const Warped &w) {
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
          tap[t] = plane_load<double>(rT, w.idx[t], o_i);
          tap[4 + t] = plane_load<double>(rT, w.idx[t], o_gx);
          tap[8 + t] = plane_load<double>(rT, w.idx[t], o_gy);
          tap[12 + t] = plane_load<double>(rT, w.idx[t], o_d);
        }
      }
    };
    auto sample = [&](const Warped &w, Sampled &s) {
      const double ax = w.ax, ay = w.ay;
      double smp[4];
#pragma unroll
      for (int c = 0; c < 4; c++)
        smp[c] = (1.0 - ay) * ((1.0 - ax) * tap[4 * c] + ax * tap[4 * c + 1]) + ay * ((1.0 - ax) * tap[4 * c + 2] + ax * tap[4 * c + 3]);
      s.i1 = smp[0]; s.gx = smp[1]; s.gy = smp[2]; s.d1 = smp[3];
      const double p00 = tap[12], p01 = tap[13], p10 = tap[14], p11 = tap[15];
      s.dgx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10);
      s.dgy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01);
      bool ok = true;
#pragma unroll
      for (int t = 0; t < 4; t++) ok = ok && (min_d < tap[12 + t]) && (tap[12 + t] < max_d);      // NaN fails
      s.taps_ok = ok;
    };
    int n_rows = 0, n_depth_rows = 0;
    auto consume = [&](const Warped &w, const Sampled &s) {
      const bool row = __builtin_amdgcn_inverse_ballot_w64(w.m);
      const double res_d = s.d1 - (cz + w.Zr);                            // D1(u, v) - Z'
      bool depth_row = row && s.taps_ok;
      if (gate_on) depth_row = depth_row && (fabs(res_d) <= gate);        // NaN fails
      n_rows += __builtin_popcountll(w.m);
      n_depth_rows += __builtin_popcountll(__builtin_amdgcn_ballot_w64(depth_row));
      if (row) {
        const double px = w.px, py = w.py, pz = w.pz, Zr = w.Zr, t25 = w.t25;
        const double res = s.i1 - w.i0;

        const double base = pz * t4 + py * t5 + px * t15;
        const double Au = base + cx;                                      // the true warp Jacobian (CORRECTED)
        const double Bv = py * t6 + pz * t9 + px * t14 + cyy;
        const double Cm = -py * t16 - pz * t17 - px * t24;                // dZ'/dpitch
        const double Dm = py * t2 - pz * t1;                              // dZ'/droll
        const double yawu = cyy - Bv, rollu = py * t4 + pz * t21, rollv = pz * t7 + py * t9;
        double J[6];
        J[0] = (s.gx * fx) * t25;
        J[1] = (s.gy * fy) * t25;
        J[2] = -(J[0] * Au + J[1] * Bv) * t25;
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
          acc[21 + a] = fma(J[a], res, acc[21 + a]);
        }
        acc[RED_COST_I] = fma(res, res, acc[RED_COST_I]);
        if (depth_row) {
          // the same six columns with the interpolant's derivative in place of the sampled gradients; dZ'/dp is
          // (0, 0, 1, 0, Cm, Dm), and since columns 4 and 5 take Cm and Dm times column 2, the -1 goes in there once
          const double rD = sigma * res_d;
          J[0] = ((sigma * s.dgx) * fx) * t25;
          J[1] = ((sigma * s.dgy) * fy) * t25;
          J[2] = -(J[0] * Au + J[1] * Bv) * t25 - sigma;
          J[3] = J[0] * yawu + J[1] * base;
          J[4] = (J[0] * cosy + J[1] * siny) * Zr + Cm * J[2];
          J[5] = J[0] * rollu + J[1] * rollv + Dm * J[2];
          q = 0;
#pragma unroll
          for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b = a; b < 6; b++) {
              acc[q] = fma(J[a], J[b], acc[q]);
              q++;
            }
            acc[21 + a] = fma(J[a], rD, acc[21 + a]);
          }
          acc[RED_COST_D] = fma(rD, rD, acc[RED_COST_D]);
        }
      }
    };
    {
      Warped w0, w1;
      Sampled s;
      int chunk = wave;                                                   // wave-uniform loop control throughout
      if (chunk < A.n_chunks) {
        warp(w0);
        issue(w0);
        for (;;) {
          chunk += NW;
          const bool more1 = chunk < A.n_chunks;
          if (more1) warp(w1);
          sample(w0, s);
          if (more1) issue(w1);
          consume(w0, s);
          if (!more1) break;
          chunk += NW;
          const bool more0 = chunk < A.n_chunks;
          if (more0) warp(w0);
          sample(w1, s);
          if (more0) issue(w0);
          consume(w1, s);
          if (!more0) break;
        }
      }
    }
    acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
    acc[RED_DEPTH_ROWS] = lane == 0 ? (double)n_depth_rows : 0.0;
    reduce_wave_to_row(acc, lane, wave, s_red);
    __syncthreads();
    if (wave == 0) {
      sum_rows_solve_update<NW>(lane, s_red, s_state, s_cst, s_ctl, A.lambda, A.max_iter, A.min_grad_norm, iteration,
                                last_gnorm, last_valid);
      // (the totals of the whole block stand in row 0 of s_red, written and read by this wave: sum_rows_broadcast)
      last_depth_rows = (int)s_red[RED_DEPTH_ROWS];
      last_cost_i = s_red[RED_COST_I];
      last_cost_d = s_red[RED_COST_D];
    }
    __syncthreads();
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
      A.reports[pair].flags |= (uint32_t)s_ctl[CTL_FLAGS];
    }
    if (B.geo_reports) {
      B.geo_reports[pair].depth_rows[A.level] = last_depth_rows;
      B.geo_reports[pair].photometric_cost[A.level] = last_cost_i;
      B.geo_reports[pair].depth_cost[A.level] = last_cost_d;
    }
    s_ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

}  // namespace

// 256-thread workgroups per CU = waves per SIMD.  One chunk's taps (32 registers) and one block of fp64 sums (64) beside two
// chunks' geometry: DESIGN.md §16 has the register figures.
constexpr int GEOMETRIC_WPS = 2;

int gn_geometric_wgs_per_cu() { return GEOMETRIC_WPS; }
int gn_geometric_lds_bytes() { return (int)lds_fixed_bytes(256); }

hipError_t gn_launch_level_geometric(const GNGeometricArgs &b, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  if (!b.geo_reports || !(b.depth_weight > 0.0)) return hipErrorInvalidValue;
  const int resident = cu_count * GEOMETRIC_WPS;                     // persistent grid: as many workgroups as stay resident
  const dim3 grid((unsigned)(b.lv.n_pairs < resident ? b.lv.n_pairs : resident)), block(256);
  hipLaunchKernelGGL((gn_level_kernel_geometric<256, GEOMETRIC_WPS>), grid, block, lds_fixed_bytes(256), stream, b);
  return hipGetLastError();
}

}  // namespace phovo_hip
