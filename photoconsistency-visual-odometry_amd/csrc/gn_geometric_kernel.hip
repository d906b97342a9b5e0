// PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC: forward-additive alignment on intensity AND depth.  Every source
// pixel that is a row of the bilinear extension with the true warp Jacobian (gn_bilinear_kernel.hip, CORRECTED; the rows of
// gn_affine_kernel.hip at alpha = beta = 0: the warp and the row of gn_sampled_device.hpp, same compile flags) contributes
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

#include "gn_sampled_device.hpp"

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
  const PairLds L = pair_lds<NW>(lds_raw);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int n = A.n, W = A.w, H = A.h;
  if (tid == 0) L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  for (;;) {                                // work queue, as in gn_level_kernel
  const int pair = pair_drawn(L);
  if (pair >= A.n_pairs) break;
  const unsigned char *src_frame = A.planes + (size_t)A.src[pair] * A.frame_bytes;
  const unsigned char *tgt_frame = A.planes + (size_t)A.tgt[pair] * A.frame_bytes;
  const __amdgpu_buffer_rsrc_t rI0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_I], n);
  const __amdgpu_buffer_rsrc_t rD0 = plane_rsrc<double>(src_frame + A.plane_off[PLANE_D], n);
  // one descriptor for the target frame; a plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(tgt_frame, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];
  const int o_d = (int)A.plane_off[PLANE_D];

  pair_begin(A, pair, wave, lane, L);

  const WarpFrame F = warp_frame(A);
  const double sigma = B.depth_weight, gate = B.max_depth_residual;
  const bool gate_on = gate > 0.0;
  const LaneWalk lw = lane_walk<NW>(wave, lane, W);

  int iteration = 0;
  double last_gnorm = 0.0, last_cost_i = 0.0, last_cost_d = 0.0;
  int last_valid = 0, last_depth_rows = 0;
  while (true) {
    const SampledPose P = sampled_pose(L.cst);

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
    int k = lw.k0;
    double cd = lw.cd0, rd = lw.rd0;
    double pz_next = plane_load<double>(rD0, k);                          // past the plane: 0
    double i0_next = plane_load<double>(rI0, k);
    auto warp = [&](Warped &w) {
      const double pz = pz_next;
      w.i0 = i0_next;
      pz_next = plane_load<double>(rD0, k + NW * WAVE);
      i0_next = plane_load<double>(rI0, k + NW * WAVE);
      clamped_taps(w.idx, warp_cell(w, warp_project(w, k, cd, rd, pz, P, F)), W, H);
      k += NW * WAVE;
      rowcol_advance(cd, rd, lw.step);
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
      for (int c = 0; c < 4; c++) smp[c] = bilerp(ax, ay, tap[4 * c], tap[4 * c + 1], tap[4 * c + 2], tap[4 * c + 3]);
      s.i1 = smp[0]; s.gx = smp[1]; s.gy = smp[2]; s.d1 = smp[3];
      const double p00 = tap[12], p01 = tap[13], p10 = tap[14], p11 = tap[15];
      s.dgx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10);
      s.dgy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01);
      bool ok = true;
#pragma unroll
      for (int t = 0; t < 4; t++) ok = ok && (F.min_d < tap[12 + t]) && (tap[12 + t] < F.max_d);      // NaN fails
      s.taps_ok = ok;
    };
    int n_rows = 0, n_depth_rows = 0;
    auto consume = [&](const Warped &w, const Sampled &s) {
      const bool row = __builtin_amdgcn_inverse_ballot_w64(w.m);
      const double res_d = s.d1 - (P.cz + w.Zr);                          // D1(u, v) - Z'
      bool depth_row = row && s.taps_ok;
      if (gate_on) depth_row = depth_row && (fabs(res_d) <= gate);        // NaN fails
      n_rows += __builtin_popcountll(w.m);
      n_depth_rows += __builtin_popcountll(__builtin_amdgcn_ballot_w64(depth_row));
      if (row) {
        const double res = s.i1 - w.i0;
        // pose_columns of gn_sampled_device.hpp, kept local and a TWIN of it: called once per row, it compiles to the same
        // instruction counts and registers as these lines but rounds differently (another choice of which product fuses
        // into an add): after several iterations poses differ in the last bit, 21 of 280 outputs of a byte comparison
        const double px = w.px, py = w.py, pz = w.pz, Zr = w.Zr, t25 = w.t25;
        const double fx = F.fx, fy = F.fy;
        const double base = pz * P.t4 + py * P.t5 + px * P.t15;
        const double Au = base + P.cx;
        const double Bv = py * P.t6 + pz * P.t9 + px * P.t14 + P.cyy;
        const double Cm = -py * P.t16 - pz * P.t17 - px * P.t24;
        const double Dm = py * P.t2 - pz * P.t1;
        const double yawu = P.cyy - Bv, rollu = py * P.t4 + pz * P.t21, rollv = pz * P.t7 + py * P.t9;
        double J[6];
        J[0] = (s.gx * fx) * t25;
        J[1] = (s.gy * fy) * t25;
        J[2] = -(J[0] * Au + J[1] * Bv) * t25;
        J[3] = J[0] * yawu + J[1] * base;
        J[4] = (J[0] * P.cosy + J[1] * P.siny) * Zr + Cm * J[2];
        J[5] = J[0] * rollu + J[1] * rollv + Dm * J[2];
        add_row(acc, J, res);
        acc[RED_COST_I] = fma(res, res, acc[RED_COST_I]);
        if (depth_row) {
          // the same six columns with the interpolant's derivative in place of the sampled gradients; dZ'/dp is
          // (0, 0, 1, 0, Cm, Dm), and since columns 4 and 5 take Cm and Dm times column 2, the -1 goes in there once
          const double rD = sigma * res_d;
          J[0] = ((sigma * s.dgx) * fx) * t25;
          J[1] = ((sigma * s.dgy) * fy) * t25;
          J[2] = -(J[0] * Au + J[1] * Bv) * t25 - sigma;
          J[3] = J[0] * yawu + J[1] * base;
          J[4] = (J[0] * P.cosy + J[1] * P.siny) * Zr + Cm * J[2];
          J[5] = J[0] * rollu + J[1] * rollv + Dm * J[2];
          add_row(acc, J, rD);
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
    reduce_wave_to_row(acc, lane, wave, L.red);
    __syncthreads();
    if (wave == 0) {
      sum_rows_solve_update<NW>(lane, L.red, L.state, L.cst, L.ctl, A.lambda, A.max_iter, A.min_grad_norm, iteration,
                                last_gnorm, last_valid);
      // (the totals of the whole block stand in row 0 of the sums, written and read by this wave: sum_rows_broadcast)
      last_depth_rows = (int)L.red[RED_DEPTH_ROWS];
      last_cost_i = L.red[RED_COST_I];
      last_cost_d = L.red[RED_COST_D];
    }
    __syncthreads();
    iteration++;
    if (L.ctl[CTL_DONE]) break;
  }
  if (tid == 0) {
    pair_report(A, pair, L, iteration, last_gnorm, last_valid);
    if (B.geo_reports) {
      B.geo_reports[pair].depth_rows[A.level] = last_depth_rows;
      B.geo_reports[pair].photometric_cost[A.level] = last_cost_i;
      B.geo_reports[pair].depth_cost[A.level] = last_cost_d;
    }
    L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
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
  return launch_persistent(gn_level_kernel_geometric<256, GEOMETRIC_WPS>, b.lv.n_pairs, cu_count, GEOMETRIC_WPS, 256,
                           lds_fixed_bytes(256), stream, b);
}

}  // namespace phovo_hip
