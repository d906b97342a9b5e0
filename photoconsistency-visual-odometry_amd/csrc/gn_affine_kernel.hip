// PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE: forward-additive alignment with a per-pair gain and offset,
//   r_k = I1(u_k, v_k) - (1 + alpha) * I0_k - beta,
// estimated jointly with the pose.  The rows are those of the bilinear extension with the true warp Jacobian
// (gn_bilinear_kernel.hip, CORRECTED): the same source pixels in raster order, the same real-valued warp, the same "in bounds
// iff the nearest pixel is" test, the same twelve clamped taps of I1, GX1 and GY1 and the same six pose columns; two columns
// are appended, dr/dalpha = -I0_k and dr/dbeta = -1.  fp64 planes only, no Huber weights.
// One pass per iteration, no scatter and no owner map, any level size; one workgroup runs all iterations of a level for a pair.
// The form is gn_level_kernel_bilinear's (taps gathered into registers), with the taps read plane by plane -- twelve 8-byte
// loads per pixel -- and one chunk's taps in flight instead of two (see the pixel loop).
// Sums: 36 + 8 + the row count.  The new columns' structure is used: beside the 21 + 6 sums of the pose block a pixel adds
//   sum J_j I0, sum J_j (j < 6), sum I0^2, sum I0, sum r I0, sum r            (16 sums; sum 1 is the row count)
// and wave 0 puts the 8 x 8 system together from them (the signs of the two columns are applied there: exact).
// The sums travel as two blocks of NRED through the analytic kernels' butterfly and fixed-order cross-wave sum, so every
// summation order depends on the level size only.
#include <hip/hip_runtime.h>

#include "gn_device.hpp"
#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

// second block of sums (slots of acc2)
enum { X_JI0 = 0, X_J = 6, X_I0I0 = 12, X_I0 = 13, X_RI0 = 14, X_R = 15 };

__host__ __device__ constexpr size_t affine_lds_bytes(int threads)
{
  return sizeof(double) * (32 + 8 + 2 * (size_t)(threads / WAVE) * NRED) + sizeof(int) * CTL_COUNT;
}

// Called by wave 0 behind the barrier that follows the two reduce_wave_to_row: sum of the NROWS rows of both blocks, the
// 8 x 8 system, solve, update, termination (sum_rows_solve_update with 8 in place of 6).
template <int NROWS>
__device__ __forceinline__ void affine_solve_update(int lane, const double *s_red, double *s_state, double *s_cst, int *s_ctl,
                                                    double lambda, int max_iter, double min_grad_norm, int iteration,
                                                    double &last_gnorm, int &last_valid)
{
  static_assert(NROWS % 2 == 0, "the rows are summed in two halves");
  double v = 0.0, u = 0.0;
  {
    const int j = lane & (NRED - 1);
    const int w0 = (lane >> 5) * (NROWS / 2);
#pragma unroll
    for (int w2 = 0; w2 < NROWS / 2; w2++) {
      v += s_red[(w0 + w2) * NRED + j];
      u += s_red[(NROWS + w0 + w2) * NRED + j];
    }
    v += __shfl_xor(v, 32, WAVE);
    u += __shfl_xor(u, 32, WAVE);
  }
  double h[36], g[NP];
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = i; j < 6; j++) h[tri8(i, j)] = __shfl(v, tri(i, j), WAVE);
    h[tri8(i, 6)] = -__shfl(u, X_JI0 + i, WAVE);
    h[tri8(i, 7)] = -__shfl(u, X_J + i, WAVE);
    g[i] = __shfl(v, 21 + i, WAVE);
  }
  const double rows = __shfl(v, RED_VALID, WAVE);
  h[tri8(6, 6)] = __shfl(u, X_I0I0, WAVE);
  h[tri8(6, 7)] = __shfl(u, X_I0, WAVE);
  h[tri8(7, 7)] = rows;
  g[6] = -__shfl(u, X_RI0, WAVE);
  g[7] = -__shfl(u, X_R, WAVE);
  last_valid = (int)rows;
  double step[NP];
  solve8_ldlt(h, g, step);
  double st[NP];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < NP; i++) {
    st[i] = s_state[i] - lambda * step[i];
    finite = finite && (fabs(st[i]) <= 1.79769313486231570815e308);
  }
  double gn2 = 0.0;
#pragma unroll
  for (int i = 0; i < NP; i++) gn2 += g[i] * g[i];
  const double gnorm = sqrt(gn2);
  bool done = false;
  if (iteration + 1 >= max_iter) done = true;
  else if (gnorm < min_grad_norm) done = true;
  if (!finite) done = true;
  if (!done) write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, lane);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NP; i++) s_state[i] = st[i];
    s_ctl[CTL_DONE] = done ? 1 : 0;
    if (!finite) s_ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_NONFINITE;
    if (last_valid < NP) s_ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_RANK_DEFICIENT;
  }
  last_gnorm = gnorm;
}

template <int T, int WPS>
__global__ __launch_bounds__(T, WPS) void gn_level_kernel_affine(const GNAffineArgs B)
{
  const GNLevelArgs &A = B.lv;
  constexpr int NW = T / WAVE;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *s_cst = reinterpret_cast<double *>(lds_raw);                 // [32]
  double *s_state = s_cst + 32;                                        // [8]: the pose, alpha, beta
  double *s_red = s_state + 8;                                         // [2][NW][NRED]
  int *s_ctl = reinterpret_cast<int *>(s_red + 2 * NW * NRED);         // [CTL_COUNT]

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

  if (wave == 0) {
    double st[6];
#pragma unroll
    for (int j = 0; j < 6; j++) st[j] = A.states[(size_t)pair * 6 + j];
    write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, lane);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 6; j++) s_state[j] = st[j];
      s_state[6] = B.illum[(size_t)pair * 2];
      s_state[7] = B.illum[(size_t)pair * 2 + 1];
      s_ctl[CTL_DONE] = 0;
      s_ctl[CTL_FLAGS] = 0;
    }
  }
  __syncthreads();

  const double fx = A.fx, fy = A.fy, ox = A.ox, oy = A.oy, ifx = A.ifx, ify = A.ify;
  const double min_d = A.min_depth, max_d = A.max_depth;
  const double wlim = (double)W - 0.5, hlim = (double)H - 0.5;
  const int k0 = wave * WAVE + lane;
  const int r0 = k0 / W, c0 = k0 - r0 * W;
  const int step_r = (NW * WAVE) / W, step_c = (NW * WAVE) - step_r * W;
  const RowColStep rc_step = make_rowcol_step(step_r, step_c, W);
  const double cd0 = (double)c0, rd0 = (double)r0;

  int iteration = 0;
  double last_gnorm = 0.0;
  int last_valid = 0;
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
    const double gain = 1.0 + uniform_f64(s_state[6]), beta = uniform_f64(s_state[7]);

    double acc[NRED], acc2[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = acc2[j] = 0.0;

    // Software pipeline over the wave's chunks.  gn_level_kernel_bilinear keeps TWO chunks' worth of taps in registers; with 44
    // sums instead of 27 that form needs more than the 256 registers two waves per SIMD leave a wave (30 spilled into the
    // pixel loop), so here ONE set of taps is in flight and the order is that of gn_level_kernel_bilinear_dma: the geometry of
    // chunk i+1 (its depth and source intensity requested a chunk earlier), then the three bilinear samples of chunk i (the
    // wait for its taps), then the twelve taps of chunk i+1 go out into the registers just freed, then the Jacobian row and
    // the 44 sums of chunk i run while they travel.  The arithmetic of a pixel is unchanged.
    struct Warped {
      double px, py, pz, Zr, t25, ax, ay, i0;
      int idx[4];                           // the clamped taps p00, p01, p10, p11: indices into a plane
      unsigned long long m;                 // lanes that are valid and land in bounds
    };
    double tap[12];                         // I1, GX1, GY1 at p00, p01, p10, p11 of the chunk whose taps are in flight
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
        }
      }
    };
    auto sample3 = [&](const Warped &w, double (&smp)[3]) {               // -> the bilinear samples I1, GX1, GY1
      const double ax = w.ax, ay = w.ay;
#pragma unroll
      for (int c = 0; c < 3; c++)
        smp[c] = (1.0 - ay) * ((1.0 - ax) * tap[4 * c] + ax * tap[4 * c + 1]) + ay * ((1.0 - ax) * tap[4 * c + 2] + ax * tap[4 * c + 3]);
    };
    int n_rows = 0;
    auto consume = [&](const Warped &w, const double (&smp)[3]) {
      n_rows += __builtin_popcountll(w.m);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
        const double px = w.px, py = w.py, pz = w.pz, Zr = w.Zr, t25 = w.t25, i0 = w.i0;
        const double res = (smp[0] - gain * i0) - beta;
        const double gxi = smp[1], gyi = smp[2];

        const double base = pz * t4 + py * t5 + px * t15;
        const double Au = base + cx;                                      // the true warp Jacobian (CORRECTED)
        const double Bv = py * t6 + pz * t9 + px * t14 + cyy;
        const double Cm = -py * t16 - pz * t17 - px * t24;
        const double Dm = py * t2 - pz * t1;
        double J[6];
        J[0] = (gxi * fx) * t25;
        J[1] = (gyi * fy) * t25;
        J[2] = -(J[0] * Au + J[1] * Bv) * t25;
        J[3] = J[0] * (cyy - Bv) + J[1] * base;
        J[4] = (J[0] * cosy + J[1] * siny) * Zr + Cm * J[2];
        J[5] = J[0] * (py * t4 + pz * t21) + J[1] * (pz * t7 + py * t9) + Dm * J[2];
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
          for (int b = a; b < 6; b++) {
            acc[q] = fma(J[a], J[b], acc[q]);
            q++;
          }
          acc[21 + a] = fma(J[a], res, acc[21 + a]);
          acc2[X_JI0 + a] = fma(J[a], i0, acc2[X_JI0 + a]);
          acc2[X_J + a] += J[a];
        }
        acc2[X_I0I0] = fma(i0, i0, acc2[X_I0I0]);
        acc2[X_I0] += i0;
        acc2[X_RI0] = fma(res, i0, acc2[X_RI0]);
        acc2[X_R] += res;
      }
    };
    {
      Warped w0, w1;
      double smp[3];
      int chunk = wave;                                                   // wave-uniform loop control throughout
      if (chunk < A.n_chunks) {
        warp(w0);
        issue(w0);
        for (;;) {
          chunk += NW;
          const bool more1 = chunk < A.n_chunks;
          if (more1) warp(w1);
          sample3(w0, smp);
          if (more1) issue(w1);
          consume(w0, smp);
          if (!more1) break;
          chunk += NW;
          const bool more0 = chunk < A.n_chunks;
          if (more0) warp(w0);
          sample3(w1, smp);
          if (more0) issue(w0);
          consume(w1, smp);
          if (!more0) break;
        }
      }
    }
    acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
    reduce_wave_to_row(acc, lane, wave, s_red);
    reduce_wave_to_row(acc2, lane, NW + wave, s_red);
    __syncthreads();
    if (wave == 0)
      affine_solve_update<NW>(lane, s_red, s_state, s_cst, s_ctl, A.lambda, A.max_iter, A.min_grad_norm, iteration,
                              last_gnorm, last_valid);
    __syncthreads();
    iteration++;
    if (s_ctl[CTL_DONE]) break;
  }
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 6; j++) A.states[(size_t)pair * 6 + j] = s_state[j];
    B.illum[(size_t)pair * 2] = s_state[6];
    B.illum[(size_t)pair * 2 + 1] = s_state[7];
    if (A.reports) {
      A.reports[pair].iterations[A.level] = iteration;
      A.reports[pair].gradient_norm = last_gnorm;
      A.reports[pair].valid_pixels[A.level] = last_valid;
      A.reports[pair].flags |= (uint32_t)s_ctl[CTL_FLAGS];
    }
    s_ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

}  // namespace

// 256-thread workgroups per CU = waves per SIMD.  One chunk's taps (24 registers) and 44 fp64 sums (88) beside two chunks'
// geometry: DESIGN.md §14 has the register figures this geometry was chosen by.
constexpr int AFFINE_WPS = 2;

int gn_affine_wgs_per_cu() { return AFFINE_WPS; }
int gn_affine_lds_bytes() { return (int)affine_lds_bytes(256); }

hipError_t gn_launch_level_affine(const GNAffineArgs &b, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  if (!b.illum) return hipErrorInvalidValue;
  const int resident = cu_count * AFFINE_WPS;                        // persistent grid: as many workgroups as stay resident
  const dim3 grid((unsigned)(b.lv.n_pairs < resident ? b.lv.n_pairs : resident)), block(256);
  hipLaunchKernelGGL((gn_level_kernel_affine<256, AFFINE_WPS>), grid, block, affine_lds_bytes(256), stream, b);
  return hipGetLastError();
}

}  // namespace phovo_hip
