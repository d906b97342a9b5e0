// Alignments behind the C ABI (include/phovo_hip.h): an enqueue's slot and its buffers, the per-level launches of the
// Gauss-Newton kernels, wait and fetch, timing and launch records.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "engine_internal.hpp"

using namespace phovo_hip;

namespace {

void free_pairs(AlignSlot &s)
{
  if (s.d_pairs) (void)hipFree(s.d_pairs);
  if (s.h_up) (void)hipHostFree(s.h_up);
  if (s.h_down) (void)hipHostFree(s.h_down);
  s.d_pairs = nullptr; s.h_up = s.h_down = nullptr; s.d_work_counters = nullptr; s.d_handover = nullptr;
  s.d_src = s.d_tgt = nullptr; s.d_states = nullptr; s.d_reports = nullptr;
  s.pair_capacity = 0;
}

// A handful of pairs on a large level: cut every pair into many workgroups (gn_wide_kernels.hip) instead of
// giving it one.  Only the reference-exact configuration (fp64 planes, no extension) takes this form.
// The forms sum in different orders, so where a level has a one-workgroup form that is fast enough -- its owner map fits LDS:
// up to ~39 k pixels, every active level of the shipped 4- and 5-level files on 640x480 -- that form runs whatever the batch
// size and a pair has ONE arithmetic (the reference has one, ...Analytic.h:500-563: Optimize() through the class surface and
// the same pair in a batch of thousands agree bit for bit); the caller may trade that for latency
// (phovo_engine_set_latency_forms).  Larger levels would take hundreds of microseconds per iteration in one workgroup:
// there a handful of pairs takes the wide form unless the caller pins the batch forms (phovo_engine_set_batch_invariant).
bool use_wide_level(const phovo_engine *e, int n_pairs, const LevelPool &lv)
{
  if (e->wide_policy < 0 || e->objective != PHOVO_OBJECTIVE_PHOTOMETRIC) return false;
  if (e->ext.plane_storage != PHOVO_STORAGE_F64 || e->ext.sampling != PHOVO_SAMPLING_NEAREST_SCATTER) return false;
  if (e->wide_policy > 0) return true;
  if (e->batch_invariant) return false;        // the automatic choice looks at the batch size
  if (n_pairs * 8 > 256) return false;
  if (lv.plan_ok && lv.plan.owner_in_lds) return e->latency_forms && lv.n >= 16384;
  return true;
}

constexpr int HEAD_SETS = 2;
// Byte offsets of the per-launch pair data for n pairs (see phovo_engine::d_pairs); every section starts 8-byte aligned.
struct PairLayout {
  size_t src, tgt, states, reports, heads, handover, handover_stride, total;
};
PairLayout pair_layout(int n_pairs)
{
  const size_t n2 = ((size_t)n_pairs + 1) & ~(size_t)1;      // two int32 per 8 bytes
  PairLayout l;
  l.src = 0;
  l.tgt = l.src + sizeof(int) * n2;
  l.states = l.tgt + sizeof(int) * n2;
  l.reports = l.states + sizeof(double) * 6 * (size_t)n_pairs;
  l.heads = l.reports + sizeof(phovo_pair_report) * (size_t)n_pairs;
  // two sets of heads per level: the sliding-window launch of a level and the exact launch behind it drain their own queues
  l.handover = l.heads + sizeof(int) * HEAD_SETS * PHOVO_MAX_LEVELS * QUEUE_HEADS_INTS;
  l.handover_stride = n2 + 2;                   // ints per level: the list of handed-over pairs and, at [n_pairs], its length
  l.total = l.handover + sizeof(int) * l.handover_stride * PHOVO_MAX_LEVELS;
  return l;
}

int ensure_pairs(AlignSlot &s, int n_pairs)
{
  if (n_pairs <= s.pair_capacity) return PHOVO_OK;
  free_pairs(s);
  const PairLayout cap = pair_layout(n_pairs);
  PHOVO_HIP_CHECK(hipMalloc(&s.d_pairs, cap.total));
  PHOVO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&s.h_up), cap.reports, hipHostMallocDefault));
  PHOVO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&s.h_down), cap.heads - cap.states, hipHostMallocDefault));
  s.pair_capacity = n_pairs;
  return PHOVO_OK;
}

constexpr int LATENCY_PAIRS = 8;     // up to this many pairs per launch the level kernels use the latency geometry

// Scratch in HBM (owner maps, ballots, the wide form's workspace) belongs to a slot, because two enqueues in flight must
// not share it -- but a caller that never has two in flight (align_pairs, the apps: one enqueue, one fetch) alternates
// between the slots and would keep TWO copies of buffers that reach gigabytes on level 0 (8192 pairs x 307 200 pixels:
// 10 GB of owner map).  So a slot that needs more than it has first looks at the OTHER slot: if that one is idle (`spare`
// is its buffer, else null), its buffer changes hands (nothing of it is in use) or, too small for this batch as well, goes
// instead of staying beside the new one; only with two enqueues really in flight does a second buffer appear.
enum class Scratch { KEPT, TAKEN, FRESH };
template <class T>
hipError_t take_or_grow(DeviceBuffer<T> &mine, DeviceBuffer<T> *spare, size_t need, Scratch *did = nullptr)
{
  const Scratch what = need <= mine.capacity ? Scratch::KEPT : spare && spare->capacity >= need ? Scratch::TAKEN : Scratch::FRESH;
  if (did) *did = what;
  if (what == Scratch::TAKEN) std::swap(mine, *spare);
  if (what != Scratch::FRESH) return hipSuccess;
  mine.release();
  if (spare) spare->release();
  return mine.reserve(need);
}

// The slot that holds enqueue `ticket`, or null when that enqueue never happened or its slot has been taken over since.
AlignSlot *slot_of(phovo_engine *e, int ticket)
{
  if (!e || ticket <= 0 || ticket > e->ticket) return nullptr;
  AlignSlot &s = e->slots[ticket % PHOVO_ENQUEUE_DEPTH];
  return s.ticket == ticket ? &s : nullptr;
}
const AlignSlot *slot_of(const phovo_engine *e, int ticket) { return slot_of(const_cast<phovo_engine *>(e), ticket); }
const char *const STALE_TICKET = "no such enqueue in flight (tickets stay valid until PHOVO_ENQUEUE_DEPTH later enqueues)";

// The records an objective keeps per pair of the last enqueue (`ran`: that enqueue ran under it), `per_pair` elements each.
template <class T>
int fetch_records(phovo_engine *e, const std::string &who, int none_status, bool AlignSlot::*ran,
                  DeviceBuffer<T> AlignSlot::*records, size_t per_pair, int n_pairs, void *out)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, who + ": null");
  AlignSlot *s = slot_of(e, e->ticket);
  if (!s) return fail(none_status, who + ": nothing has been enqueued");
  if (!(s->*ran)) return fail(PHOVO_E_UNSUPPORTED, who + ": the last enqueue ran under another objective");
  if (n_pairs != s->last_pairs) return fail(PHOVO_E_INVALID_ARGUMENT, who + ": n_pairs differs from that enqueue's");
  if (n_pairs == 0) return PHOVO_OK;
  if (!out) return fail(PHOVO_E_INVALID_ARGUMENT, who + ": null");
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(hipStreamSynchronize(s->stream));
  PHOVO_HIP_CHECK(hipMemcpy(out, (s->*records).ptr, sizeof(T) * per_pair * (size_t)n_pairs, hipMemcpyDeviceToHost));
  return PHOVO_OK;
}

}  // namespace

void phovo_hip::free_slot(AlignSlot &s)
{
  free_pairs(s);
  s.owner.release();
  s.mask.release();
  s.wide_ws.release();
  s.tr_reports.release();
  s.illum.release();
  s.geo_reports.release();
  s.rob_reports.release();
  s.sd_reports.release();
  s.sd_records.release();
  s.prior.release();
  s.prior_reports.release();
  if (s.h_prior) (void)hipHostFree(s.h_prior);
  s.h_prior = nullptr; s.h_prior_capacity = 0;
}

extern "C" {

int phovo_engine_level_uses_wide(const phovo_engine *e, int level, int n_pairs)
{
  if (!e || level < 0 || level >= e->cfg.num_levels || e->n_frames == 0) return 0;
  if (e->objective != PHOVO_OBJECTIVE_PHOTOMETRIC) return 0;
  return use_wide_level(e, n_pairs, e->levels[level]) && !(e->ext.huber_delta[level] > 0.0) ? 1 : 0;
}

// phovo_engine_enqueue_align and, with `with_prior`, phovo_engine_enqueue_align_prior.
static int enqueue(phovo_engine *e, int n_pairs, const int *source_frames, const int *target_frames,
                   const double *init_states, bool with_prior, const double *prior_states, const double *information)
{
  if (!e || !source_frames || !target_frames) return fail(PHOVO_E_INVALID_ARGUMENT, "align: null");
  if (n_pairs < 0) return fail(PHOVO_E_INVALID_ARGUMENT, "align: n_pairs < 0");
  if (with_prior) {
    if (e->objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL && e->objective != PHOVO_OBJECTIVE_INVERSE_ROBUST)   // (7: a follow-up)
      return fail(PHOVO_E_UNSUPPORTED, "align_prior: the pose prior belongs to the two inverse-compositional objectives "
                                       "(PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL, PHOVO_OBJECTIVE_INVERSE_ROBUST)");
    if (n_pairs > 0 && (!prior_states || !information)) return fail(PHOVO_E_INVALID_ARGUMENT, "align_prior: null");
    for (size_t i = 0; i < (size_t)n_pairs * 6; i++)
      if (!std::isfinite(prior_states[i])) return fail(PHOVO_E_INVALID_ARGUMENT, "align_prior: a prior state is not finite");
    for (size_t i = 0; i < (size_t)n_pairs * 36; i++)
      if (!std::isfinite(information[i])) return fail(PHOVO_E_INVALID_ARGUMENT, "align_prior: an information entry is not finite");
    for (size_t i = 0; i < (size_t)n_pairs; i++)
      for (int d = 0; d < 6; d++)
        if (information[i * 36 + (size_t)d * 7] < 0.0)
          return fail(PHOVO_E_INVALID_ARGUMENT, "align_prior: an information matrix has a negative diagonal entry");
  }
  if (e->n_frames == 0) return fail(PHOVO_E_NOT_READY, "align: no frames resident (reserve_frames and upload first; set_config, set_extensions and set_objective drop the pool when its layout changes)");
  if (!e->have_K) return fail(PHOVO_E_NOT_READY, "align: SetIntrinsicMatrix has not been called");
  for (int i = 0; i < n_pairs; i++) {
    if (source_frames[i] < 0 || source_frames[i] >= e->n_frames || target_frames[i] < 0 || target_frames[i] >= e->n_frames)
      return fail(PHOVO_E_INVALID_ARGUMENT, "align: frame index out of range");
  }
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  // Every active level must be launchable BEFORE the enqueue takes a ticket and a slot: a refused enqueue leaves the
  // engine as it was -- in particular the results of the enqueue before the last stay fetchable.
  size_t owner_need = 0, wide_need = 0, mask_need = 0, sd_slab = 0;
  for (int l = 0; l < e->cfg.num_levels && n_pairs > 0; l++) {
    if (e->cfg.max_num_iterations[l] <= 0) continue;
    const LevelPool &lv = e->levels[l];
    if (!lv.stored) return fail(PHOVO_E_NOT_READY, "align: an active level is not resident");
    if (e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE) {
      if (!lv.plan_bi_ok)
        return fail(PHOVO_E_SHAPE, "align: pyramid level too large for the bi-objective (more than 2 097 151 pixels)");
      if (!lv.plan_bi.owner_in_lds) owner_need = std::max(owner_need, (size_t)n_pairs * (size_t)lv.n);
      continue;
    }
    if (e->objective == PHOVO_OBJECTIVE_TRUST_REGION) {
      if (!lv.plan_tr_ok)
        return fail(PHOVO_E_SHAPE, "align: pyramid level too large for the trust-region objective (more than 2 097 151 pixels)");
      // (one map per resident workgroup: the persistent grid, not the batch)
      const size_t wgs = (size_t)std::min(n_pairs, e->cu_count * lv.plan_tr.wgs_per_cu);
      if (!lv.plan_tr.owner_in_lds) owner_need = std::max(owner_need, wgs * (size_t)lv.n);
      continue;
    }
    if (e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE) continue;       // no owner map, no LDS limit
    if (e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) {            // likewise; the target's depth is a source upload's
      for (int i = 0; i < n_pairs; i++)
        if (!(e->frame_roles[(size_t)target_frames[i] * PHOVO_MAX_LEVELS + (size_t)l] & PHOVO_ROLE_SOURCE))
          return fail(PHOVO_E_NOT_READY, "align: the photometric-geometric objective reads the target's depth (upload target "
                                         "frames with PHOVO_ROLE_BOTH)");
      continue;
    }
    if (e->objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL || e->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST ||
        e->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {                // likewise; the source's gradients are a target upload's
      for (int i = 0; i < n_pairs; i++)
        if (!(e->frame_roles[(size_t)source_frames[i] * PHOVO_MAX_LEVELS + (size_t)l] & PHOVO_ROLE_TARGET))
          return fail(PHOVO_E_NOT_READY, "align: the inverse-compositional objective reads the source's gradient planes (upload "
                                         "source frames with PHOVO_ROLE_BOTH)");
      if (e->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {
        if (lv.w > 65535 || lv.h > 65535)
          return fail(PHOVO_E_SHAPE, "align: the semi-dense objective's pixel records hold 16-bit columns and rows (a level wider "
                                     "or taller than 65535 pixels)");
        sd_slab = std::max(sd_slab, gn_inverse_semidense_slab_records((lv.n + 63) / 64));
      }
      continue;
    }
    if (e->ext.sampling == PHOVO_SAMPLING_BILINEAR) continue;       // no owner map, no LDS limit
    const bool wide = use_wide_level(e, n_pairs, lv) && !(e->ext.huber_delta[l] > 0.0);
    if (wide) {
      const size_t ws = gn_wide_workspace_bytes(lv.n, n_pairs);
      if (ws > wide_need) wide_need = ws;
    }
    if (!wide && !lv.plan_ok)
      return fail(PHOVO_E_SHAPE, "align: pyramid level too large for the device path (more than 2 097 151 pixels: the owner map in "
                                 "HBM holds 21-bit source indices); up to 32 pairs at a time take the wide form, which has no such limit");
    if (wide || !lv.plan.owner_in_lds) {
      const size_t need = (size_t)n_pairs * (size_t)lv.n;
      if (need > owner_need) owner_need = need;
    }
    if (!wide && lv.plan.mask_in_hbm) {
      const size_t need = (size_t)n_pairs * (size_t)((lv.n + 63) / 64);
      if (need > mask_need) mask_need = need;
    }
  }
  // The slot this enqueue takes: the one used least recently.  Its previous enqueue (ticket - PHOVO_ENQUEUE_DEPTH) must
  // have finished -- its pinned mirror and pair data are about to be rewritten -- but the enqueue before this one may
  // still be running: it lives in the other slot, on the other stream.
  const int ticket = e->ticket + 1;
  AlignSlot &s = e->slots[ticket % PHOVO_ENQUEUE_DEPTH];
  PHOVO_HIP_CHECK(hipStreamSynchronize(s.stream));
  // From here on the slot's previous content is gone.  It holds NO enqueue until this one has been issued completely: a
  // failure on the way (an allocation, a launch) leaves a slot that every ticket-taking entry point refuses, instead of one
  // that hands out whatever an earlier enqueue left in its buffers.
  s.ticket = 0;
  s.last_pairs = n_pairs;
  s.have_timing = false;
  s.launches.clear();
  for (bool &b : s.level_launched) b = false;
  s.d_states = nullptr;
  s.tr_ran = e->objective == PHOVO_OBJECTIVE_TRUST_REGION;
  s.affine_ran = e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE;
  s.geometric_ran = e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC;
  s.robust_ran = e->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST;
  s.semidense_ran = e->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE;
  s.prior_ran = with_prior;
  s.num_levels = e->cfg.num_levels;
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++) s.level_skipped[l] = l < e->cfg.num_levels && e->cfg.max_num_iterations[l] <= 0;
  if (n_pairs == 0) {                    // nothing to run: a valid, empty enqueue (fetch of 0 pairs succeeds, no device buffer)
    e->ticket = ticket;
    s.ticket = ticket;
    return PHOVO_OK;
  }
  // planes written on the engine's own stream so far (uploads return synchronised; plane setters too): nothing to order --
  // except behind a device ingest, which returns while the pyramids are still being built
  if (e->ingest_pending) PHOVO_HIP_CHECK(hipStreamWaitEvent(s.stream, e->ev_ingested, 0));
  int st = ensure_pairs(s, n_pairs);
  if (st != PHOVO_OK) return st;

  // scratch in HBM: the slot's own, the idle other slot's, or new (take_or_grow)
  AlignSlot &other = e->slots[(ticket + 1) % PHOVO_ENQUEUE_DEPTH];
  const bool other_idle = other.stream && hipStreamQuery(other.stream) == hipSuccess;
  Scratch owner_is;
  PHOVO_HIP_CHECK(take_or_grow(s.owner, other_idle ? &other.owner : nullptr, owner_need, &owner_is));
  if (owner_is == Scratch::TAKEN) std::swap(s.owner_tagged, other.owner_tagged);
  if (owner_is == Scratch::FRESH) {
    s.owner_tagged = false;
    // -1 everywhere once: the wide form restores -1 after every iteration, the persistent kernel wipes per pair
    PHOVO_HIP_CHECK(fill_i32(s.owner.ptr, owner_need, -1, s.stream));
  }
  PHOVO_HIP_CHECK(take_or_grow(s.mask, other_idle ? &other.mask : nullptr, mask_need));
  PHOVO_HIP_CHECK(take_or_grow(s.wide_ws, other_idle ? &other.wide_ws : nullptr, wide_need));
  if (wide_need) s.h_wide_done.resize((size_t)n_pairs * 4);
  if (s.tr_ran) PHOVO_HIP_CHECK(s.tr_reports.reserve((size_t)n_pairs));
  if (s.affine_ran) PHOVO_HIP_CHECK(s.illum.reserve(2 * (size_t)n_pairs));
  if (s.geometric_ran) PHOVO_HIP_CHECK(s.geo_reports.reserve((size_t)n_pairs));
  if (s.robust_ran) PHOVO_HIP_CHECK(s.rob_reports.reserve((size_t)n_pairs));
  if (s.semidense_ran) {
    PHOVO_HIP_CHECK(s.sd_reports.reserve((size_t)n_pairs));
    // one slab per workgroup of the persistent grid (the same grid on every level)
    const size_t grid = (size_t)std::min(n_pairs, e->cu_count * gn_inverse_semidense_wgs_per_cu());
    PHOVO_HIP_CHECK(take_or_grow(s.sd_records, other_idle ? &other.sd_records : nullptr, grid * sd_slab));
  }
  if (s.prior_ran) {
    const size_t doubles = (size_t)GN_PRIOR_DOUBLES * (size_t)n_pairs;
    PHOVO_HIP_CHECK(s.prior.reserve(doubles));
    PHOVO_HIP_CHECK(s.prior_reports.reserve((size_t)n_pairs));
    if (doubles > s.h_prior_capacity) {
      if (s.h_prior) (void)hipHostFree(s.h_prior);
      s.h_prior = nullptr; s.h_prior_capacity = 0;
      PHOVO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&s.h_prior), sizeof(double) * doubles, hipHostMallocDefault));
      s.h_prior_capacity = doubles;
    }
    // a pair's block: eigenPose(prior state) as (R_p, t_p), Lambda's upper triangle, and whether Lambda has an entry at all
    for (int i = 0; i < n_pairs; i++) {
      const double *ps = prior_states + (size_t)i * 6, *li = information + (size_t)i * 36;
      double *b = s.h_prior + (size_t)i * GN_PRIOR_DOUBLES;
      const double sy = std::sin(ps[3]), cy = std::cos(ps[3]), sp = std::sin(ps[4]), cp = std::cos(ps[4]);
      const double sr = std::sin(ps[5]), cr = std::cos(ps[5]);
      b[0] = cy * cp; b[1] = cy * sp * sr - sy * cr; b[2] = cy * sp * cr + sy * sr;
      b[3] = sy * cp; b[4] = sy * sp * sr + cy * cr; b[5] = sy * sp * cr - cy * sr;
      b[6] = -sp;     b[7] = cp * sr;                b[8] = cp * cr;
      b[9] = ps[0]; b[10] = ps[1]; b[11] = ps[2];
      bool any = false;
      int k = 12;
      for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) {
          b[k++] = li[r * 6 + c];
          any = any || li[r * 6 + c] != 0.0;
        }
      b[k] = any ? 1.0 : 0.0;
    }
  }
  // The caller may reuse its arrays as soon as this returns and the copies below are asynchronous: the slot's pinned
  // mirror keeps them alive until the slot is used again (synchronised above).
  const PairLayout lay = pair_layout(n_pairs);
  s.d_src = reinterpret_cast<int *>(s.d_pairs + lay.src);
  s.d_tgt = reinterpret_cast<int *>(s.d_pairs + lay.tgt);
  s.d_states = reinterpret_cast<double *>(s.d_pairs + lay.states);
  s.d_reports = reinterpret_cast<phovo_pair_report *>(s.d_pairs + lay.reports);
  s.d_work_counters = reinterpret_cast<int *>(s.d_pairs + lay.heads);
  s.d_handover = reinterpret_cast<int *>(s.d_pairs + lay.handover);
  std::memset(s.h_up, 0, lay.reports);
  std::memcpy(s.h_up + lay.src, source_frames, sizeof(int) * (size_t)n_pairs);
  std::memcpy(s.h_up + lay.tgt, target_frames, sizeof(int) * (size_t)n_pairs);
  if (init_states)                                                                   // SetInitialStateVector  :494
    std::memcpy(s.h_up + lay.states, init_states, sizeof(double) * 6 * (size_t)n_pairs);
  // one copy in (pair list + initial states, zeros without them), one memset (reports + the work-queue heads of all levels)
  PHOVO_HIP_CHECK(hipMemcpyAsync(s.d_pairs, s.h_up, lay.reports, hipMemcpyHostToDevice, s.stream));
  PHOVO_HIP_CHECK(hipMemsetAsync(s.d_pairs + lay.reports, 0, lay.total - lay.reports, s.stream));
  if (s.tr_ran)          // (every level the configuration skips stays PHOVO_TR_SKIPPED = 0)
    PHOVO_HIP_CHECK(hipMemsetAsync(s.tr_reports.ptr, 0, sizeof(phovo_trust_region_report) * (size_t)n_pairs, s.stream));
  if (s.affine_ran)      // every pair starts at alpha = beta = 0
    PHOVO_HIP_CHECK(hipMemsetAsync(s.illum.ptr, 0, sizeof(double) * 2 * (size_t)n_pairs, s.stream));
  if (s.geometric_ran)   // (every level the configuration skips stays 0)
    PHOVO_HIP_CHECK(hipMemsetAsync(s.geo_reports.ptr, 0, sizeof(phovo_geometric_report) * (size_t)n_pairs, s.stream));
  if (s.robust_ran)      // (likewise)
    PHOVO_HIP_CHECK(hipMemsetAsync(s.rob_reports.ptr, 0, sizeof(phovo_robust_report) * (size_t)n_pairs, s.stream));
  if (s.semidense_ran)   // (likewise)
    PHOVO_HIP_CHECK(hipMemsetAsync(s.sd_reports.ptr, 0, sizeof(phovo_semidense_report) * (size_t)n_pairs, s.stream));
  if (s.prior_ran) {
    PHOVO_HIP_CHECK(hipMemcpyAsync(s.prior.ptr, s.h_prior, sizeof(double) * GN_PRIOR_DOUBLES * (size_t)n_pairs,
                                   hipMemcpyHostToDevice, s.stream));
    PHOVO_HIP_CHECK(hipMemsetAsync(s.prior_reports.ptr, 0, sizeof(phovo_prior_report) * (size_t)n_pairs, s.stream));
  }
  PHOVO_HIP_CHECK(hipEventRecord(s.ev_total_start, s.stream));

  auto record = [&](int first, int last, int kind, int threads, int lds, int wgs) {
    phovo_launch_record r{};
    r.level_first = first; r.level_last = last; r.kind = kind; r.threads = threads; r.lds_bytes = lds; r.workgroups = wgs;
    s.launches.push_back(r);
  };
  auto persistent_grid = [&](int wgs_per_cu) { const int slots = e->cu_count * wgs_per_cu; return n_pairs < slots ? n_pairs : slots; };
  auto level_args = [&](int l) {
    GNLevelArgs a{};
    fill_level_view(a, e, l);
    a.level = l;
    a.max_iter = e->cfg.max_num_iterations[l];
    a.lambda = e->cfg.lambda_optimization_step[l];
    a.min_grad_norm = e->cfg.min_gradient_norm[l];
    a.huber_delta = e->ext.huber_delta[l];
    a.rec_off = e->levels[l].rec_off;
    a.src = s.d_src; a.tgt = s.d_tgt;
    a.states = s.d_states; a.reports = s.d_reports;
    a.g_owner = s.owner.ptr;
    a.n_pairs = n_pairs;
    a.work_counter = s.d_work_counters + l * QUEUE_HEADS_INTS;
    // one queue per XCD once there are enough pairs to keep every XCD's share of the grid busy
    a.n_queues = (!tuning_switch("PHOVO_QUEUE_SINGLE") && n_pairs >= 8 * 64) ? QUEUES_PER_LEVEL : 1;
    return a;
  };
  // a handful of pairs leaves most CUs empty: such a batch takes the geometry with the shorter iteration
  const bool few_batch = e->latency_forms && !e->batch_invariant && n_pairs <= LATENCY_PAIRS;
  // Can level l be one of several levels of ONE launch (gn_fused_kernel)?  The persistent scatter kernel with its owner map
  // in half a CU's LDS; not the latency geometry of a small batch, not the wide form.
  auto fusable = [&](int l) {
    const LevelPool &lv = e->levels[l];
    if (e->fusion == PHOVO_FUSION_OFF || e->ext.sampling == PHOVO_SAMPLING_BILINEAR || few_batch) return false;
    if (e->objective != PHOVO_OBJECTIVE_PHOTOMETRIC) return false;
    if (use_wide_level(e, n_pairs, lv) && !(e->ext.huber_delta[l] > 0.0)) return false;
    return gn_level_fusable(lv.n);
  };

  int split_until = -1;        // PHOVO_FUSION_SPLIT: the levels down to this one belong to the run whose first launch has gone out
  for (int l = e->cfg.num_levels - 1; l >= 0; l--) {                                 // coarse to fine  :502-503
    if (e->cfg.max_num_iterations[l] <= 0) continue;                                 // :526 (nothing observable happens)
    const LevelPool &lv = e->levels[l];
    GNLevelArgs a = level_args(l);
    PHOVO_HIP_CHECK(hipEventRecord(s.ev_start[l], s.stream));

    // Data-dependent termination (a gradient threshold on any of them): the run of consecutive fusable levels that starts
    // here goes out as ONE persistent launch in which every pair flows through those levels inside the workgroup that drew
    // it.  Which levels form a run depends on the configuration and the level sizes only, never on the batch (apart from
    // the latency forms of batches of <= 8 pairs, which batch_invariant switches off): see phovo_engine_set_batch_invariant.
    // With thresholds of zero every pair runs max_num_iterations and a level boundary costs nothing: one launch per level,
    // each in its own best geometry.
    if (fusable(l)) {
      int run[GN_MAX_FUSED_LEVELS], n_run = 0;
      bool data_dependent = false;
      for (int m = l; m >= 0 && n_run < GN_MAX_FUSED_LEVELS; m--) {
        if (e->cfg.max_num_iterations[m] <= 0) continue;
        if (!fusable(m)) break;
        run[n_run++] = m;
        if (e->cfg.min_gradient_norm[m] > 0.0) data_dependent = true;
      }
      if (l >= split_until && split_until >= 0) { n_run = 2; data_dependent = true; }        // a later level of a split run
      else if (n_run >= 2 && data_dependent && e->fusion == PHOVO_FUSION_SPLIT) split_until = run[n_run - 1];
      if (n_run >= 2 && data_dependent && e->fusion == PHOVO_FUSION_AUTO) {
        GNFusedArgs f{};
        f.n_levels = n_run; f.n_pairs = n_pairs; f.n_queues = a.n_queues; f.work_counter = a.work_counter;
        for (int i = 0; i < n_run; i++) {
          f.lv[i] = level_args(run[i]);
          if (f.lv[i].n > f.n_max) f.n_max = f.lv[i].n;
        }
        PHOVO_HIP_CHECK(gn_launch_fused(f, e->ext.plane_storage, e->cu_count, s.stream));
        record(l, run[n_run - 1], PHOVO_LAUNCH_FUSED, 512, gn_fused_lds_bytes(f.n_max), persistent_grid(2));
        PHOVO_HIP_CHECK(hipEventRecord(s.ev_stop[l], s.stream));
        s.level_launched[l] = true;
        l = run[n_run - 1];                        // (the loop's l-- moves on to the level below the run)
        continue;
      }
      if (n_run >= 2 && data_dependent && e->fusion == PHOVO_FUSION_SPLIT) {
        // the fused geometry, one launch per level: what a fused run is bit-identical to (tests)
        GNLaunchPlan mid{};
        (void)gn_plan_fused_geometry(lv.n, &mid);
        PHOVO_HIP_CHECK(gn_launch_level(a, mid, e->ext.plane_storage, e->cu_count, s.stream));
        record(l, l, PHOVO_LAUNCH_PERSISTENT, mid.threads, mid.lds_bytes, persistent_grid(mid.wgs_per_cu));
        PHOVO_HIP_CHECK(hipEventRecord(s.ev_stop[l], s.stream));
        s.level_launched[l] = true;
        continue;
      }
    }

    if (e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE) {
      GNBiObjectiveArgs b{};
      b.lv = a;
      b.dgx_off = lv.dgx_off; b.dgy_off = lv.dgy_off; b.gain_off = lv.gain_off;
      PHOVO_HIP_CHECK(gn_launch_level_biobjective(b, lv.plan_bi, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_BIOBJECTIVE, lv.plan_bi.threads, lv.plan_bi.lds_bytes, persistent_grid(lv.plan_bi.wgs_per_cu));
      if (!lv.plan_bi.owner_in_lds) s.owner_tagged = true;    // tagged entries stay behind (the kernel wipes per pair)
    } else if (e->objective == PHOVO_OBJECTIVE_TRUST_REGION) {
      GNTrustRegionArgs b{};
      b.lv = a;
      const phovo_trust_region_options &o = e->tr_opt;
      b.lv.fx = e->K[0] / std::pow(2.0, l); b.lv.fy = e->K[4] / std::pow(2.0, l);      // Ceres.h:164-169: divisions
      b.lv.ox = e->K[2] / std::pow(2.0, l); b.lv.oy = e->K[5] / std::pow(2.0, l);
      b.lv.ifx = 1.0 / b.lv.fx; b.lv.ify = 1.0 / b.lv.fy;
      b.max_iterations = e->cfg.max_num_iterations[l];
      b.function_tolerance = o.function_tolerance[l]; b.gradient_tolerance = o.gradient_tolerance[l];
      b.parameter_tolerance = o.parameter_tolerance[l];
      b.initial_radius = o.initial_trust_region_radius[l]; b.max_radius = o.max_trust_region_radius[l];
      b.min_radius = o.min_trust_region_radius[l]; b.min_relative_decrease = o.min_relative_decrease[l];
      b.tr_reports = s.tr_reports.ptr;
      PHOVO_HIP_CHECK(gn_launch_level_trust_region(b, lv.plan_tr, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_TRUST_REGION, lv.plan_tr.threads, lv.plan_tr.lds_bytes, persistent_grid(lv.plan_tr.wgs_per_cu));
      if (!lv.plan_tr.owner_in_lds) s.owner_tagged = true;    // tagged entries stay behind (the kernel wipes per pair)
    } else if (e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE) {
      GNAffineArgs b{};
      b.lv = a;
      b.illum = s.illum.ptr;
      PHOVO_HIP_CHECK(gn_launch_level_affine(b, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_AFFINE, 256, gn_affine_lds_bytes(), persistent_grid(gn_affine_wgs_per_cu()));
    } else if (e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) {
      GNGeometricArgs b{};
      b.lv = a;
      b.depth_weight = e->geo_opt.depth_weight[l];
      b.max_depth_residual = e->geo_opt.max_depth_residual[l];
      b.geo_reports = s.geo_reports.ptr;
      PHOVO_HIP_CHECK(gn_launch_level_geometric(b, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_GEOMETRIC, 256, gn_geometric_lds_bytes(), persistent_grid(gn_geometric_wgs_per_cu()));
    } else if (s.prior_ran) {                        // objective 5 or 6 (checked at the top)
      const bool robust = e->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST;
      GNInversePriorArgs b{};
      b.lv = a;
      b.scale_factor = e->rob_opt.scale_factor;
      b.rob_reports = robust ? s.rob_reports.ptr : nullptr;
      b.prior = s.prior.ptr;
      b.prior_reports = s.prior_reports.ptr;
      b.level_scale = e->prior_opt.level_scale[l];
      PHOVO_HIP_CHECK(gn_launch_level_inverse_prior(b, robust, e->cu_count, s.stream));
      record(l, l, robust ? PHOVO_LAUNCH_INVERSE_ROBUST_PRIOR : PHOVO_LAUNCH_INVERSE_PRIOR, 256,
             gn_inverse_prior_lds_bytes(robust), persistent_grid(gn_inverse_prior_wgs_per_cu()));
    } else if (e->objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL) {
      GNInverseArgs b{};
      b.lv = a;
      PHOVO_HIP_CHECK(gn_launch_level_inverse(b, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_INVERSE, 256, gn_inverse_lds_bytes(), persistent_grid(gn_inverse_wgs_per_cu()));
    } else if (e->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST) {
      GNInverseRobustArgs b{};
      b.lv = a;
      b.scale_factor = e->rob_opt.scale_factor;
      b.rob_reports = s.rob_reports.ptr;
      PHOVO_HIP_CHECK(gn_launch_level_inverse_robust(b, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_INVERSE_ROBUST, 256, gn_inverse_robust_lds_bytes(), persistent_grid(gn_inverse_robust_wgs_per_cu()));
    } else if (e->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {
      GNInverseSemiDenseArgs b{};
      b.lv = a;
      b.tau2 = e->sd_opt.min_pixel_gradient[l] * e->sd_opt.min_pixel_gradient[l];
      b.records = s.sd_records.ptr;
      b.slab_records = sd_slab;
      b.seg_records = gn_inverse_semidense_segment_records(a.n_chunks);
      b.sd_reports = s.sd_reports.ptr;
      PHOVO_HIP_CHECK(gn_launch_level_inverse_semidense(b, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_INVERSE_SEMIDENSE, 256, gn_inverse_semidense_lds_bytes(),
             persistent_grid(gn_inverse_semidense_wgs_per_cu()));
    } else if (e->ext.sampling == PHOVO_SAMPLING_BILINEAR) {
      PHOVO_HIP_CHECK(gn_launch_level_bilinear(a, e->ext.plane_storage, e->ext.jacobian_corrected != 0, e->cu_count, s.stream));
      record(l, l, PHOVO_LAUNCH_BILINEAR, 256, 0, persistent_grid(gn_bilinear_wgs_per_cu(e->ext.plane_storage)));
    } else if (use_wide_level(e, n_pairs, lv) && !(e->ext.huber_delta[l] > 0.0)) {
      if (s.owner_tagged) {            // the wide form starts from -1 everywhere and leaves it so
        PHOVO_HIP_CHECK(fill_i32(s.owner.ptr, s.owner.capacity, -1, s.stream));
        s.owner_tagged = false;
      }
      PHOVO_HIP_CHECK(gn_run_level_wide(a, n_pairs, s.wide_ws.ptr, s.h_wide_done.data(), s.stream));
      record(l, l, PHOVO_LAUNCH_WIDE, 256, 0, n_pairs * ((lv.n + 1023) / 1024));
    } else {
      const bool few = few_batch && lv.plan_few_ok && lv.plan_few.owner_in_lds == lv.plan.owner_in_lds;
      const GNLaunchPlan &pl = few ? lv.plan_few : lv.plan;
      a.n_lds = pl.owner_in_lds ? 0 : pl.owner_lds_entries;
      a.g_mask = pl.mask_in_hbm ? s.mask.ptr : nullptr;
      a.depth_lds_chunks = pl.depth_lds_chunks;
      int *list0 = s.d_handover + (size_t)l * lay.handover_stride;
      int *heads1 = s.d_work_counters + (PHOVO_MAX_LEVELS + l) * QUEUE_HEADS_INTS;
      // (tuning build: the sliding-window kernel also on levels whose owner map fits LDS, from 160x120 up -- an A/B, profiles/r04_runs)
      const bool slide_anyway = tuning_switch("PHOVO_SLIDE_FROM_160x120") && lv.n >= 19200 && !few;
      if ((!pl.owner_in_lds || slide_anyway) && e->slide_policy >= 0) {
        // Owner map too large for LDS: the sliding-window kernel first (owner ring in LDS); pairs whose warp leaves its
        // window are put on the hand-over list and continued, from the iteration they had reached, by the exact kernel
        // right behind it, which draws from that list.
        a.handover_out = list0;
        a.slide_m = gn_slide_reach_bands(lv.w, lv.h);
        PHOVO_HIP_CHECK(gn_launch_level_slide(a, e->ext.plane_storage, e->cu_count, s.stream));
        record(l, l, PHOVO_LAUNCH_SLIDE, gn_slide_threads(), (int)gn_slide_lds_bytes(), persistent_grid(1));
        a.handover_out = nullptr; a.handover_in = list0; a.takeover_flag = PHOVO_PAIR_WINDOW_FALLBACK;
        a.work_counter = heads1; a.n_queues = 1;
        PHOVO_HIP_CHECK(gn_launch_level(a, pl, e->ext.plane_storage, e->cu_count, s.stream));
        record(l, l, PHOVO_LAUNCH_SLIDE_FALLBACK, pl.threads, pl.lds_bytes, persistent_grid(pl.wgs_per_cu));
        s.owner_tagged = true;                              // tagged entries stay behind (the kernel wipes per pair)
      } else {
        PHOVO_HIP_CHECK(gn_launch_level(a, pl, e->ext.plane_storage, e->cu_count, s.stream));
        record(l, l, PHOVO_LAUNCH_PERSISTENT, pl.threads, pl.lds_bytes, persistent_grid(pl.wgs_per_cu));
        if (!pl.owner_in_lds) s.owner_tagged = true;
      }
    }
    PHOVO_HIP_CHECK(hipEventRecord(s.ev_stop[l], s.stream));
    s.level_launched[l] = true;
  }
  PHOVO_HIP_CHECK(hipEventRecord(s.ev_total_stop, s.stream));
  s.have_timing = true;
  e->ticket = ticket;                  // issued completely: the enqueue exists
  s.ticket = ticket;
  return PHOVO_OK;
}

int phovo_engine_enqueue_align(phovo_engine *e, int n_pairs, const int *source_frames,
                               const int *target_frames, const double *init_states)
{
  return enqueue(e, n_pairs, source_frames, target_frames, init_states, false, nullptr, nullptr);
}

int phovo_engine_enqueue_align_prior(phovo_engine *e, int n_pairs, const int *source_frames, const int *target_frames,
                                     const double *init_states, const double *prior_states, const double *information)
{
  return enqueue(e, n_pairs, source_frames, target_frames, init_states, true, prior_states, information);
}

int phovo_engine_last_ticket(const phovo_engine *e) { return e ? e->ticket : 0; }

int phovo_engine_last_launches(const phovo_engine *e, phovo_launch_record *out, int capacity, int *count)
{
  if (!e || !count) return fail(PHOVO_E_INVALID_ARGUMENT, "last_launches: null");
  const AlignSlot *s = slot_of(e, e->ticket);
  *count = s ? (int)s->launches.size() : 0;
  if (out && s)
    for (int i = 0; i < capacity && i < *count; i++) out[i] = s->launches[(size_t)i];
  return PHOVO_OK;
}

int phovo_engine_synchronize(phovo_engine *e)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "synchronize: null");
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  e->ingest_pending = false;
  PHOVO_HIP_CHECK(quiesce(e));
  return PHOVO_OK;
}

int phovo_engine_wait(phovo_engine *e, int ticket)
{
  AlignSlot *s = slot_of(e, ticket);
  if (!s) return fail(PHOVO_E_INVALID_ARGUMENT, std::string("wait: ") + STALE_TICKET);
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(hipStreamSynchronize(s->stream));
  return PHOVO_OK;
}

int phovo_engine_fetch(phovo_engine *e, int ticket, int n_pairs, double *out_states, phovo_pair_report *reports)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "fetch: null");
  AlignSlot *s = slot_of(e, ticket);
  if (!s) return fail(PHOVO_E_INVALID_ARGUMENT, std::string("fetch: ") + STALE_TICKET);
  if (n_pairs != s->last_pairs) return fail(PHOVO_E_INVALID_ARGUMENT, "fetch: n_pairs differs from that enqueue's");
  if (n_pairs == 0) return PHOVO_OK;
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  const PairLayout pl = pair_layout(n_pairs);
  // one copy out: states (and reports right behind them, when asked for) into pinned memory
  const size_t bytes = (reports ? pl.heads : pl.reports) - pl.states;
  PHOVO_HIP_CHECK(hipMemcpyAsync(s->h_down, s->d_pairs + pl.states, bytes, hipMemcpyDeviceToHost, s->stream));
  PHOVO_HIP_CHECK(hipStreamSynchronize(s->stream));
  if (out_states) std::memcpy(out_states, s->h_down, sizeof(double) * 6 * (size_t)n_pairs);
  if (reports) {
    std::memcpy(reports, s->h_down + (pl.reports - pl.states), sizeof(phovo_pair_report) * (size_t)n_pairs);
    // Levels with max_num_iterations == 0 still run the loop body once in the reference (:510,547-549).  (The Ceres
    // aligner skips them: 0 steps.)  The levels are those of the configuration the ENQUEUE ran under: with two enqueues
    // in flight the caller may have set another one since.
    for (int i = 0; i < n_pairs && !s->tr_ran; i++)
      for (int l = 0; l < s->num_levels; l++)
        if (s->level_skipped[l]) reports[i].iterations[l] = 1;
  }
  return PHOVO_OK;
}

int phovo_engine_fetch_trust_region_reports(phovo_engine *e, int n_pairs, phovo_trust_region_report *reports)
{
  return fetch_records(e, "fetch_trust_region_reports", PHOVO_E_INVALID_ARGUMENT, &AlignSlot::tr_ran, &AlignSlot::tr_reports, 1,
                       n_pairs, reports);
}

int phovo_engine_fetch_illumination(phovo_engine *e, int n_pairs, double *alpha_beta)
{
  return fetch_records(e, "fetch_illumination", PHOVO_E_NOT_READY, &AlignSlot::affine_ran, &AlignSlot::illum, 2, n_pairs,
                       alpha_beta);
}

int phovo_engine_fetch_geometric_reports(phovo_engine *e, int n_pairs, phovo_geometric_report *reports)
{
  return fetch_records(e, "fetch_geometric_reports", PHOVO_E_NOT_READY, &AlignSlot::geometric_ran, &AlignSlot::geo_reports, 1,
                       n_pairs, reports);
}

int phovo_engine_fetch_robust_reports(phovo_engine *e, int n_pairs, phovo_robust_report *reports)
{
  return fetch_records(e, "fetch_robust_reports", PHOVO_E_NOT_READY, &AlignSlot::robust_ran, &AlignSlot::rob_reports, 1, n_pairs,
                       reports);
}

int phovo_engine_fetch_semidense_reports(phovo_engine *e, int n_pairs, phovo_semidense_report *reports)
{
  return fetch_records(e, "fetch_semidense_reports", PHOVO_E_NOT_READY, &AlignSlot::semidense_ran, &AlignSlot::sd_reports, 1,
                       n_pairs, reports);
}

int phovo_engine_fetch_prior_reports(phovo_engine *e, int n_pairs, phovo_prior_report *reports)
{
  return fetch_records(e, "fetch_prior_reports", PHOVO_E_NOT_READY, &AlignSlot::prior_ran, &AlignSlot::prior_reports, 1, n_pairs,
                       reports);
}

int phovo_engine_fetch_results(phovo_engine *e, int n_pairs, double *out_states, phovo_pair_report *reports)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "fetch_results: null");
  if (e->ticket == 0) return n_pairs == 0 ? PHOVO_OK : fail(PHOVO_E_INVALID_ARGUMENT, "fetch_results: nothing has been enqueued");
  return phovo_engine_fetch(e, e->ticket, n_pairs, out_states, reports);
}

int phovo_engine_device_states(phovo_engine *e, int ticket, void **states)
{
  if (!e || !states) return fail(PHOVO_E_INVALID_ARGUMENT, "device_states: null");
  AlignSlot *s = slot_of(e, ticket);
  if (!s) return fail(PHOVO_E_INVALID_ARGUMENT, std::string("device_states: ") + STALE_TICKET);
  *states = s->d_states;
  return PHOVO_OK;
}

int phovo_engine_results_device_ptr(phovo_engine *e, void **states)
{
  if (!e || !states) return fail(PHOVO_E_INVALID_ARGUMENT, "results_device_ptr: null");
  const AlignSlot *s = slot_of(e, e->ticket);
  *states = s ? s->d_states : nullptr;
  return PHOVO_OK;
}

int phovo_engine_align_pairs(phovo_engine *e, int n_pairs, const int *source_frames,
                             const int *target_frames, const double *init_states,
                             double *out_states, phovo_pair_report *reports)
{
  int st = phovo_engine_enqueue_align(e, n_pairs, source_frames, target_frames, init_states);
  if (st != PHOVO_OK) return st;
  return phovo_engine_fetch_results(e, n_pairs, out_states, reports);
}

int phovo_engine_align_ms(const phovo_engine *e, int ticket, double *total_ms, double level_ms[PHOVO_MAX_LEVELS])
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "align_ms: null");
  const AlignSlot *s = slot_of(e, ticket);
  if (!s || !s->have_timing) return fail(PHOVO_E_NOT_READY, "align_ms: nothing has been enqueued under that ticket");
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(hipStreamSynchronize(s->stream));
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++) {
    double ms = 0;
    if (s->level_launched[l]) {
      float f = 0;
      PHOVO_HIP_CHECK(hipEventElapsedTime(&f, s->ev_start[l], s->ev_stop[l]));
      ms = f;
    }
    if (level_ms) level_ms[l] = ms;
  }
  if (total_ms) {           // first launch to last
    float f = 0;
    PHOVO_HIP_CHECK(hipEventElapsedTime(&f, s->ev_total_start, s->ev_total_stop));
    *total_ms = f;
  }
  return PHOVO_OK;
}

int phovo_engine_last_align_ms(const phovo_engine *e, double *total_ms, double level_ms[PHOVO_MAX_LEVELS])
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "last_align_ms: null");
  if (e->ticket == 0) return fail(PHOVO_E_NOT_READY, "last_align_ms: nothing has been enqueued");
  return phovo_engine_align_ms(e, e->ticket, total_ms, level_ms);
}

int phovo_engine_level_launch_info(const phovo_engine *e, int level, int *threads, int *lds_bytes,
                                   int *owner_in_lds, int *source_in_lds)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "level_launch_info: null");
  if (level < 0 || level >= e->cfg.num_levels) return fail(PHOVO_E_INVALID_ARGUMENT, "level out of range");
  if (e->n_frames == 0) return fail(PHOVO_E_NOT_READY, "no frame pool reserved");
  const LevelPool &lv = e->levels[level];
  if (!lv.plan_ok) return fail(PHOVO_E_SHAPE, "level too large for the device path");
  if (!lv.plan.owner_in_lds && e->slide_policy >= 0) {       // the sliding-window kernel runs first on such a level
    if (threads) *threads = gn_slide_threads();
    if (lds_bytes) *lds_bytes = (int)gn_slide_lds_bytes();
    if (owner_in_lds) *owner_in_lds = 0;                     // a ring of 32768 entries, not the whole map
    if (source_in_lds) *source_in_lds = 0;
    return PHOVO_OK;
  }
  if (threads) *threads = lv.plan.threads;
  if (lds_bytes) *lds_bytes = lv.plan.lds_bytes;
  if (owner_in_lds) *owner_in_lds = lv.plan.owner_in_lds ? 1 : 0;
  if (source_in_lds) *source_in_lds = lv.plan.source_in_lds ? 1 : 0;
  return PHOVO_OK;
}

}  // extern "C"
