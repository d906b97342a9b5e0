// PHOVO_OBJECTIVE_INVERSE_ROBUST: the inverse-compositional aligner of gn_inverse_kernel.hip under a Huber
// weight whose threshold follows the pair's own residuals,
//   delta = scale_factor * median |r|,     w = |r| <= delta ? 1 : delta / |r|,     H = sum w J J^T,   g = sum w J r.
// Rows, residual, Jacobian row, solve, composition, termination and the level's exit are that kernel's, through the same
// helpers (gn_sampled_device.hpp, gn_inverse_device.hpp).
// TWIN: the pixel loop (Warped, warp_issue, the two-chunk pipeline around consume) stands in gn_level_kernel_inverse too, and
// this whole kernel -- that loop, the histogram and the median scan -- a second time in gn_inverse_prior_kernel.hip (the form
// with a pose prior); a change goes into all three.  It is restated, not shared, so that objective 5's code
// stays what it was.
// The median is the grouped-data median of a histogram in LDS: 4096 bins of width 2^-12 over |r|, filled with LDS integer
// atomic adds while the rows are consumed, so the counts -- and with them every bit of the result -- do not depend on the
// order in which the lanes arrive.  The threshold lags one iteration: a histogram-only pass at the level's entry pose gives
// delta_0; iteration i weights with delta_i and histograms its own residuals, from which delta_{i+1} comes.  One pass over
// the pixels per iteration, as before, and one more per level.
// The scan: thread t owns bins 16 t .. 16 t + 15, reads and clears them, and the 256 sums are scanned inside each wave;
// the four wave totals cross in LDS, and the one thread whose bins hold the median writes delta.  A bin's word sits at
// bin ^ ((bin >> 6) & 15): thread t's j-th bin then lies in bank 16 (t & 3) + (j ^ (t >> 2)) and the 64 lanes of a read or a
// store touch 64 different banks.
#include <hip/hip_runtime.h>

#include "gn_inverse_device.hpp"

namespace phovo_hip {

namespace {

constexpr int ROBUST_BINS = 4096;
constexpr int RED_OUTLIERS = 28;          // slot behind the row count (RED_VALID): the rows with |r| > delta, as exact as the row count
static_assert(RED_VALID < RED_OUTLIERS && RED_OUTLIERS < NRED, "one block of NRED carries every sum");

// The kernel's STATIC LDS, beside the dynamic lds_fixed_bytes of every level kernel: the histogram, the threshold of the next
// system and the four waves' counts.  (Static, so the code object's metadata states it: tests/test_kernel_structure_inverse_robust.py.)
struct alignas(16) RobustLds {         // (the dynamic block behind it is 16-byte aligned)
  unsigned hist[ROBUST_BINS];             // swizzled (hist_word)
  double delta;
  int wave_total[4];
};
static_assert(sizeof(RobustLds) == 16 * 1024 + 32, "16 KiB of histogram, six words, padding to 16 bytes");

__device__ __forceinline__ int hist_word(int bin) { return bin ^ ((bin >> 6) & 15); }

template <int T, int WPS>
__global__ __launch_bounds__(T, WPS) void gn_level_kernel_inverse_robust(const GNInverseRobustArgs B)
{
  const GNLevelArgs &A = B.lv;
  constexpr int NW = T / WAVE;
  static_assert(T * 16 == ROBUST_BINS && NW == 4, "a thread owns 16 bins; four wave totals");
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PairLds L = pair_lds<NW>(lds_raw);
  __shared__ RobustLds X;

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int W = A.w, H = A.h;
  const double scale = B.scale_factor;
#pragma unroll
  for (int j = 0; j < 16; j++) X.hist[hist_word(16 * tid + j)] = 0u;      // every pass leaves it clear again (pair_drawn has the barrier)
  if (tid == 0) L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  for (;;) {                                // work queue, as in gn_level_kernel
  const int pair = pair_drawn(L);
  if (pair >= A.n_pairs) break;
  // one descriptor per frame; a plane is chosen by the load's scalar offset
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(A.planes + (size_t)A.src[pair] * A.frame_bytes, A.frame_bytes);
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(A.planes + (size_t)A.tgt[pair] * A.frame_bytes, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_d = (int)A.plane_off[PLANE_D];
  const int o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];

  pair_begin(A, pair, wave, lane, L);       // the block holds eigenPose(state): the (R, t) this level starts from

  const WarpFrame F = warp_frame(A);
  const LaneWalk lw = lane_walk<NW>(wave, lane, W);

  int iteration = 0;
  double last_gnorm = 0.0, delta = 0.0;
  int last_valid = 0, last_outliers = 0;
  bool build = false;                       // the first pass at the entry pose fills the histogram only: delta_0
  while (true) {
    const SampledPose P = sampled_pose_rt(L.cst);
    if (build) delta = uniform_f64(X.delta);                             // delta_i: from the pass before this one

    double acc[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = 0.0;

    // The software pipeline of gn_level_kernel_inverse (see there): two chunks' taps in flight.
    struct Warped {
      double px, py, pz, Zr, t25, ax, ay, i0, gx, gy;
      double tap[4];                        // I1 at p00, p01, p10, p11
      unsigned long long m;                 // lanes that are valid and land in bounds
    };
    int k = lw.k0;
    double cd = lw.cd0, rd = lw.rd0;
    double pz_next = plane_load<double>(rS, k, o_d), i0_next = plane_load<double>(rS, k, o_i);
    double gx_next = plane_load<double>(rS, k, o_gx), gy_next = plane_load<double>(rS, k, o_gy);
    auto warp_issue = [&](Warped &w) {
      const double pz = pz_next;
      w.i0 = i0_next; w.gx = gx_next; w.gy = gy_next;
      pz_next = plane_load<double>(rS, k + NW * WAVE, o_d);
      i0_next = plane_load<double>(rS, k + NW * WAVE, o_i);
      gx_next = plane_load<double>(rS, k + NW * WAVE, o_gx);
      gy_next = plane_load<double>(rS, k + NW * WAVE, o_gy);
      int idx[4];
      clamped_taps(idx, warp_cell(w, warp_project(w, k, cd, rd, pz, P, F)), W, H);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
        for (int t = 0; t < 4; t++) w.tap[t] = plane_load<double>(rT, idx[t], o_i);
      }
      k += NW * WAVE;
      rowcol_advance(cd, rd, lw.step);
    };
    int n_rows = 0;                         // the wave's rows (wave-uniform)
    int n_out = 0;                          // THIS LANE's rows beyond delta: counted under the row mask, so per lane
    auto consume = [&](const Warped &w) {
      n_rows += __builtin_popcountll(w.m);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {                     // rows only: nothing else is counted
        const double res = bilerp(w.ax, w.ay, w.tap[0], w.tap[1], w.tap[2], w.tap[3]) - w.i0;
        const double ar = fabs(res);
        const double q = ar * 4096.0;
        const int bin = q < 4096.0 ? (int)q : ROBUST_BINS - 1;            // 0 <= q < 4096 in the first arm; 1 and above, and NaN: the last bin
        __hip_atomic_fetch_add(&X.hist[hist_word(bin)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (build) {
          n_out += ar > delta ? 1 : 0;
          const double wgt = ar <= delta ? 1.0 : delta / ar;
          double J[6], Jw[6];
          inverse_row(J, w.gx, w.gy, w.px, w.py, w.pz, F.fx, F.fy);
#pragma unroll
          for (int i = 0; i < 6; i++) Jw[i] = wgt * J[i];
          add_row(acc, Jw, J, res);
        }
      }
    };
    {
      Warped w0, w1;
      int chunk = wave;                                                   // wave-uniform loop control throughout
      if (chunk < A.n_chunks) {
        warp_issue(w0);
        for (;;) {
          chunk += NW;
          const bool more1 = chunk < A.n_chunks;
          if (more1) warp_issue(w1);
          consume(w0);
          if (!more1) break;
          chunk += NW;
          const bool more0 = chunk < A.n_chunks;
          if (more0) warp_issue(w0);
          consume(w1);
          if (!more0) break;
        }
      }
    }
    if (build) {
      acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
      acc[RED_OUTLIERS] = (double)n_out;                                  // (the butterfly adds the lanes up: exact)
      reduce_wave_to_row(acc, lane, wave, L.red);
    }
    lds_barrier();                          // every count of the pass is in

    if (build && wave == 0) {
      inverse_solve_compose<NW>(lane, L, A.lambda, A.max_iter, A.min_grad_norm, iteration, last_gnorm, last_valid);
      last_outliers = (int)L.red[RED_OUTLIERS];                           // (sum_rows_broadcast left every total in row 0)
    }

    // This thread's 16 bins, in order, out of the histogram and zero behind them; the inclusive scan of the 64 sums of the
    // wave.  (The order of the scan changes no value: integers.)
    int cnt[16];
#pragma unroll
    for (int j = 0; j < 16; j++) cnt[j] = (int)X.hist[hist_word(16 * tid + j)];
#pragma unroll
    for (int j = 0; j < 16; j++) X.hist[hist_word(16 * tid + j)] = 0u;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) mine += cnt[j];
    int incl = mine;
#pragma unroll
    for (int d = 1; d < WAVE; d *= 2) {
      const int up = __shfl_up(incl, d, WAVE);
      if (lane >= d) incl += up;
    }
    if (lane == WAVE - 1) X.wave_total[wave] = incl;
    __syncthreads();

    // The median rule, by the one thread whose bins take the cumulative count to `half`: delta of the NEXT system.
    {
      int below = 0, n = 0;
#pragma unroll
      for (int w2 = 0; w2 < NW; w2++) {
        const int t = X.wave_total[w2];
        below += w2 < wave ? t : 0;
        n += t;
      }
      const int half = (n + 1) / 2;
      const int last = below + incl;        // the cumulative count through this thread's bins
      int before = last - mine;
      if (n == 0) {
        if (tid == 0) X.delta = scale * 0.0;
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
        X.delta = scale * m;
      }
    }
    __syncthreads();
    if (!build) { build = true; continue; }                               // the entry pass: no system, no iteration
    iteration++;
    if (L.ctl[CTL_DONE]) break;
  }
  if (tid == 0) {
    pair_report(A, pair, L, iteration, last_gnorm, last_valid);
    B.rob_reports[pair].delta[A.level] = delta;
    B.rob_reports[pair].outliers[A.level] = last_outliers;
    L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

}  // namespace

// 256-thread workgroups per CU = waves per SIMD, as gn_level_kernel_inverse: DESIGN.md §22 has the compiled figures.
constexpr int INVERSE_ROBUST_WPS = 2;

int gn_inverse_robust_wgs_per_cu() { return INVERSE_ROBUST_WPS; }
int gn_inverse_robust_lds_bytes() { return (int)(lds_fixed_bytes(256) + sizeof(RobustLds)); }

hipError_t gn_launch_level_inverse_robust(const GNInverseRobustArgs &b, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  if (!b.rob_reports || !(b.scale_factor > 0.0)) return hipErrorInvalidValue;
  return launch_persistent(gn_level_kernel_inverse_robust<256, INVERSE_ROBUST_WPS>, b.lv.n_pairs, cu_count, INVERSE_ROBUST_WPS,
                           256, lds_fixed_bytes(256), stream, b);
}

}  // namespace phovo_hip
