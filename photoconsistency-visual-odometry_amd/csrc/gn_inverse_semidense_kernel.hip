// PHOVO_OBJECTIVE_INVERSE_SEMIDENSE: the inverse-compositional aligner on SELECTED source pixels.  A Jacobian
// row of that aligner depends on the source pixel alone (gn_inverse_kernel.hip), so which pixels are worth a row is decided
// ONCE per pair and level, before the first iteration:
//   pixel k is selected  iff  min_depth < D0_k < max_depth  and  GX0_k^2 + GY0_k^2 >= tau_L^2     (fp64, NaN fails either),
// and the rows of an iteration are the selected pixels whose warp lands in bounds.  Everything behind the selection --
// warp_project, the bounds test, clamped_taps, bilerp, the residual, inverse_row, add_row, inverse_solve_compose, termination
// and the level's exit -- is objective 5's, from gn_sampled_device.hpp and gn_inverse_device.hpp: the objective IS objective 5
// on a source whose depth is NaN wherever the pixel is not selected (tests/semidense_ref.py).  The order of summation is this
// kernel's own (a lane meets the selected pixels in list order, not at a fixed stride), so the two agree within rounding.
// Level entry: behind pair_begin every wave walks ITS chunks of D0, GX0, GY0 (the chunk walk of gn_level_kernel_inverse:
// chunks wave, wave + NW, ...), coalesced, and compacts the selected pixels of a chunk behind those of its earlier chunks:
// ballot of the selected lanes, rank = popcount of the ballot below the lane, a running wave-uniform count.  A wave writes
// its own SEGMENT of the workgroup's slab and later reads that segment alone: no scan across waves, no atomics, the order
// fixed by the walk.  A record is 4 bytes, col | row << 16 (levels wider or taller than 65535 are refused by the host).
// Workspace (GNInverseSemiDenseArgs::records, owned by the enqueue's slot): [grid][slab_records] records, the slab indexed by
// blockIdx.x, a wave's segment seg_records = 64 * ceil(n_chunks / NW) records at wave * seg_records in it; slab_records is
// NW * seg_records of the LARGEST active level of the enqueue.  4 bytes x padded level size x grid: 640x480 on 512
// workgroups is 0.63 GB.  A slab keeps the previous pair's records behind the current counts: nothing reads them (below).
// Iterations: a wave walks its segment 64 records at a time -- one coalesced record load, four gathers D0, I0, GX0, GY0 at
// the pixel, warp_project with ((double)col, (double)row), four gathered taps, the row and the 28 sums -- software-pipelined
// as in the TWIN: the records of chunk i + 2, the source values of chunk i + 1 and the taps of chunk i are in flight while
// chunk i - 1 is consumed.  The records are read through a buffer descriptor whose extent is the wave's COUNT, so a lane at or
// past the count reads record 0 (pixel 0, always a legal gather) whatever the slab holds there, and the row mask drops it.
// TWIN: the consume side (Warped, the taps under the mask, consume, the two-chunk alternation) is gn_inverse_kernel.hip's
// pixel loop; a change to it there is looked at here.
#include <hip/hip_runtime.h>

#include "gn_inverse_device.hpp"          // se3_exp, euler_from_rotation_lane0, inverse_solve_compose

namespace phovo_hip {

namespace {

template <int T, int WPS>
__global__ __launch_bounds__(T, WPS) void gn_level_kernel_inverse_semidense(const GNInverseSemiDenseArgs B)
{
  const GNLevelArgs &A = B.lv;
  constexpr int NW = T / WAVE;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PairLds L = pair_lds<NW>(lds_raw);
  int *const s_count = L.ctl + CTL_COUNT;   // [NW] records per wave, for the report

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int W = A.w, H = A.h;
  // this wave's segment of this workgroup's slab
  unsigned *const seg = B.records + (size_t)blockIdx.x * B.slab_records + (size_t)wave * (size_t)B.seg_records;
  if (tid == 0) L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  for (;;) {                                // work queue, as in gn_level_kernel
  const int pair = pair_drawn(L);
  if (pair >= A.n_pairs) break;
  const __amdgpu_buffer_rsrc_t rS = frame_rsrc(A.planes + (size_t)A.src[pair] * A.frame_bytes, A.frame_bytes);
  const __amdgpu_buffer_rsrc_t rT = frame_rsrc(A.planes + (size_t)A.tgt[pair] * A.frame_bytes, A.frame_bytes);
  const int o_i = (int)A.plane_off[PLANE_I], o_d = (int)A.plane_off[PLANE_D];
  const int o_gx = (int)A.plane_off[PLANE_GX], o_gy = (int)A.plane_off[PLANE_GY];

  pair_begin(A, pair, wave, lane, L);       // the block holds eigenPose(state): the (R, t) this level starts from

  const WarpFrame F = warp_frame(A);

  // ---- level entry: the list of this pair's selected pixels ----
  int count = 0;                            // (wave-uniform) records in this wave's segment: starts at 0 for EVERY pair
  {
    const LaneWalk lw = lane_walk<NW>(wave, lane, W);
    int k = lw.k0;
    double cd = lw.cd0, rd = lw.rd0;
    double d_next = plane_load<double>(rS, k, o_d);
    double gx_next = plane_load<double>(rS, k, o_gx), gy_next = plane_load<double>(rS, k, o_gy);
    for (int chunk = wave; chunk < A.n_chunks; chunk += NW) {             // wave-uniform loop control
      const double d = d_next, gx = gx_next, gy = gy_next;
      // (a chunk ahead; past the plane the read is the frame's next plane or 0 and nobody uses it)
      d_next = plane_load<double>(rS, k + NW * WAVE, o_d);
      gx_next = plane_load<double>(rS, k + NW * WAVE, o_gx);
      gy_next = plane_load<double>(rS, k + NW * WAVE, o_gy);
      const bool sel = k < A.n && F.min_d < d && d < F.max_d && gx * gx + gy * gy >= B.tau2;
      const unsigned long long b = __builtin_amdgcn_ballot_w64(sel);
      // selected lanes BELOW this one (the lane's own bit is not counted)
      const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      // count + rank < 64 * (chunks of this wave so far) <= seg_records: inside the segment
      if (sel) seg[count + rank] = (unsigned)(int)cd | ((unsigned)(int)rd << 16);
      count += __builtin_popcountll(b);
      k += NW * WAVE;
      rowcol_advance(cd, rd, lw.step);
    }
  }
  count = __builtin_amdgcn_readfirstlane(count);
  if (lane == 0) s_count[wave] = count;     // read by thread 0 behind the barriers of the first iteration
  // Every store of the list has completed before the wave's first read of it (the wave reads only what it wrote itself:
  // nothing crosses waves, so no barrier).  The stores are plain global stores and the reads go through a buffer
  // descriptor; both pass the CU's one vector L1 with the default cache policy, and the list rests on a wave's own program
  // order through that cache.  Whoever gives either side another policy (nontemporal, sc bits, an LDS-DMA read) has to
  // give the other the same or put a cache write-back / invalidate between them: no test would notice the difference
  // on a lucky run.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // the segment as far as it is valid: a record index at or past `count` reads 0
  const __amdgpu_buffer_rsrc_t rL = __builtin_amdgcn_make_buffer_rsrc(seg, 0, count * (int)sizeof(unsigned), 0x00020000);
  const int n_list_chunks = (count + WAVE - 1) / WAVE;

  int iteration = 0;
  double last_gnorm = 0.0;
  int last_valid = 0;
  while (true) {
    const SampledPose P = sampled_pose_rt(L.cst);

    double acc[NRED];
#pragma unroll
    for (int j = 0; j < NRED; j++) acc[j] = 0.0;

    struct Warped {
      double px, py, pz, Zr, t25, ax, ay, i0, gx, gy;
      double tap[4];                        // I1 at p00, p01, p10, p11
      unsigned long long m;                 // lanes that hold a record, are valid and land in bounds
    };
    auto record_load = [&](int j) {         // record j of the segment; 0 at or past the count
      return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rL, j * (int)sizeof(unsigned), 0, 0);
    };
    auto pixel_of = [&](unsigned rec) { return __mul24((int)(rec >> 16), W) + (int)(rec & 0xffffu); };
    // rec_a: the records whose four source values are in flight (*_next); rec_b: the records of the chunk behind them
    int j = lane;                           // this lane's record index in the chunk that warp_issue takes next
    unsigned rec_a = record_load(j), rec_b = record_load(j + WAVE);
    double pz_next, i0_next, gx_next, gy_next;
    {
      const int k = pixel_of(rec_a);
      pz_next = plane_load<double>(rS, k, o_d); i0_next = plane_load<double>(rS, k, o_i);
      gx_next = plane_load<double>(rS, k, o_gx); gy_next = plane_load<double>(rS, k, o_gy);
    }
    auto warp_issue = [&](Warped &w) {
      const double pz = pz_next;
      w.i0 = i0_next; w.gx = gx_next; w.gy = gy_next;
      const unsigned rec = rec_a;
      const unsigned long long listed = __builtin_amdgcn_ballot_w64(j < count);
      rec_a = rec_b;
      rec_b = record_load(j + 2 * WAVE);
      {
        const int kn = pixel_of(rec_a);
        pz_next = plane_load<double>(rS, kn, o_d); i0_next = plane_load<double>(rS, kn, o_i);
        gx_next = plane_load<double>(rS, kn, o_gx); gy_next = plane_load<double>(rS, kn, o_gy);
      }
      const int col = (int)(rec & 0xffffu), row = (int)(rec >> 16);
      int idx[4];
      const WarpTarget tg = warp_project(w, __mul24(row, W) + col, (double)col, (double)row, pz, P, F);
      w.m &= listed;
      clamped_taps(idx, warp_cell(w, tg), W, H);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
#pragma unroll
        for (int t = 0; t < 4; t++) w.tap[t] = plane_load<double>(rT, idx[t], o_i);
      }
      j += WAVE;
    };
    int n_rows = 0;
    auto consume = [&](const Warped &w) {
      n_rows += __builtin_popcountll(w.m);
      if (__builtin_amdgcn_inverse_ballot_w64(w.m)) {
        const double res = bilerp(w.ax, w.ay, w.tap[0], w.tap[1], w.tap[2], w.tap[3]) - w.i0;
        double J[6];
        inverse_row(J, w.gx, w.gy, w.px, w.py, w.pz, F.fx, F.fy);
        add_row(acc, J, res);
      }
    };
    {
      Warped w0, w1;
      int chunk = 0;                                                      // wave-uniform loop control throughout
      if (chunk < n_list_chunks) {
        warp_issue(w0);
        for (;;) {
          chunk++;
          const bool more1 = chunk < n_list_chunks;
          if (more1) warp_issue(w1);
          consume(w0);
          if (!more1) break;
          chunk++;
          const bool more0 = chunk < n_list_chunks;
          if (more0) warp_issue(w0);
          consume(w1);
          if (!more0) break;
        }
      }
    }
    acc[RED_VALID] = lane == 0 ? (double)n_rows : 0.0;
    reduce_wave_to_row(acc, lane, wave, L.red);
    __syncthreads();
    if (wave == 0)
      inverse_solve_compose<NW>(lane, L, A.lambda, A.max_iter, A.min_grad_norm, iteration, last_gnorm, last_valid);
    __syncthreads();
    iteration++;
    if (L.ctl[CTL_DONE]) break;
  }
  if (tid == 0) {
    pair_report(A, pair, L, iteration, last_gnorm, last_valid);
    int selected = 0;
#pragma unroll
    for (int w2 = 0; w2 < NW; w2++) selected += s_count[w2];
    B.sd_reports[pair].selected[A.level] = selected;
    L.ctl[CTL_PAIR] = draw_pair(A.work_counter, A.n_queues, A.n_pairs);
  }
  }   // next pair
}

constexpr size_t semidense_lds_bytes() { return lds_fixed_bytes(256) + sizeof(int) * (256 / WAVE); }

}  // namespace

// 256-thread workgroups per CU = waves per SIMD, chosen from the compiled kernel's register count: DESIGN.md §25 has the
// figures.
constexpr int INVERSE_SEMIDENSE_WPS = 2;

int gn_inverse_semidense_wgs_per_cu() { return INVERSE_SEMIDENSE_WPS; }
int gn_inverse_semidense_lds_bytes() { return (int)semidense_lds_bytes(); }
int gn_inverse_semidense_segment_records(int n_chunks) { return WAVE * ((n_chunks + 256 / WAVE - 1) / (256 / WAVE)); }
size_t gn_inverse_semidense_slab_records(int n_chunks)
{
  return (size_t)(256 / WAVE) * (size_t)gn_inverse_semidense_segment_records(n_chunks);
}

hipError_t gn_launch_level_inverse_semidense(const GNInverseSemiDenseArgs &b, int cu_count, hipStream_t stream)
{
  if (b.lv.n_pairs <= 0) return hipSuccess;
  return launch_persistent(gn_level_kernel_inverse_semidense<256, INVERSE_SEMIDENSE_WPS>, b.lv.n_pairs, cu_count,
                           INVERSE_SEMIDENSE_WPS, 256, semidense_lds_bytes(), stream, b);
}

}  // namespace phovo_hip
