// What the host files behind the C ABI share (host only; no kernel sees any of it): the engine and its parts, and the few
// helpers more than one of them needs.
//   engine.cpp           lifecycle, configuration, frame pool, uploads, device ingest, plane access
//   engine_align.cpp     enqueue, wait and fetch, timing and launch records
//   engine_evaluate.cpp  the systems at given poses (phovo_engine_evaluate_*_pairs)
//   odometry_c.cpp       the single-pair class surface (phovo_odometry_*), a client of the engine
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "phovo_internal.hpp"

#define PHOVO_HIP_CHECK(expr)                                                                   \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return fail(PHOVO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));              \
  } while (0)

namespace phovo_hip {

struct LevelPool {
  int w = 0, h = 0, n = 0;
  bool stored = false;
  unsigned char *planes = nullptr;   // frame f at planes + f*frame_bytes, plane p of it at + plane_off[p]
  size_t frame_bytes = 0;
  size_t plane_off[PLANES_PER_FRAME] = {0, 0, 0, 0};
  size_t rec_off = 0;                  // bilinear sampling: the frame's tap records {I, GX, GY, pad} behind its planes (0: none)
  // bi-objective: the target's depth-gradient planes and its depth gain behind the four planes (0: none)
  size_t dgx_off = 0, dgy_off = 0, gain_off = 0;
  GNLaunchPlan plan_bi{};
  bool plan_bi_ok = false;
  GNLaunchPlan plan_tr{};              // trust-region objective
  bool plan_tr_ok = false;
  GNLaunchPlan plan{};
  bool plan_ok = false;
  GNLaunchPlan plan_few{};             // geometry for a handful of pairs (LATENCY_PAIRS or fewer)
  bool plan_few_ok = false;
};

// A device allocation of `capacity` elements that only grows: reserve(n) keeps it when it is large enough and otherwise
// frees it first and allocates n (the content is lost).  A plain value: copies alias, std::swap hands it over, and
// whoever owns it calls release().
template <class T>
struct DeviceBuffer {
  T *ptr = nullptr;
  size_t capacity = 0;
  hipError_t reserve(size_t n)
  {
    if (n <= capacity) return hipSuccess;
    release();
    const hipError_t he = hipMalloc(&ptr, sizeof(T) * n);
    if (he == hipSuccess) capacity = n;
    return he;
  }
  void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; capacity = 0; }
};

}  // namespace phovo_hip

// Everything ONE enqueue owns: its stream, its pair data, its scratch and its timing events.  The engine keeps
// PHOVO_ENQUEUE_DEPTH of them and uses them in turn, so that enqueue k + 1 can be issued -- and its kernels can start filling
// the CUs that enqueue k's last, long pairs leave idle -- before enqueue k has finished (phovo_hip.h, "Pipelining").
struct AlignSlot {
  hipStream_t stream = nullptr;
  hipEvent_t ev_total_start = nullptr, ev_total_stop = nullptr;
  hipEvent_t ev_start[PHOVO_MAX_LEVELS] = {};
  hipEvent_t ev_stop[PHOVO_MAX_LEVELS] = {};
  bool level_launched[PHOVO_MAX_LEVELS] = {};
  bool have_timing = false;
  int ticket = 0;                              // the enqueue this slot holds (0: none yet)
  int last_pairs = 0;
  // Per-launch pair data in ONE device allocation, laid out for the pairs of the enqueue as
  //   [src int32 | tgt int32 | states fp64 x6 | reports | work-queue heads | hand-over lists]
  // so that an enqueue is one host-to-device copy (src, tgt, initial states, from the pinned mirror h_up) and one
  // memset (reports + heads + lists), and a fetch is one device-to-host copy (states + reports, into the pinned h_down).
  int pair_capacity = 0;
  unsigned char *d_pairs = nullptr;
  unsigned char *h_up = nullptr, *h_down = nullptr;      // pinned
  int *d_src = nullptr, *d_tgt = nullptr;                // views into d_pairs for the enqueue
  double *d_states = nullptr;
  phovo_pair_report *d_reports = nullptr;
  int *d_work_counters = nullptr;              // [2][PHOVO_MAX_LEVELS][QUEUES_PER_LEVEL x QUEUE_HEAD_STRIDE] work-queue heads of the level launches (view into d_pairs)
  int *d_handover = nullptr;                   // [PHOVO_MAX_LEVELS][pairs + 2] hand-over lists: sliding-window kernel -> exact kernel (view into d_pairs)
  phovo_hip::DeviceBuffer<int> owner;          // owner maps in HBM (levels whose map exceeds LDS; the wide form)
  phovo_hip::DeviceBuffer<unsigned long long> mask;      // in-bounds ballots in HBM (levels whose ballots do not fit LDS next to the rest)
  bool owner_tagged = false;                   // `owner` holds tagged entries of the persistent kernel, not the -1 the wide form expects
  phovo_hip::DeviceBuffer<unsigned char> wide_ws;        // workspace of the wide (many-workgroups-per-pair) level form
  std::vector<int> h_wide_done;
  std::vector<phovo_launch_record> launches;   // what the enqueue launched, in order (phovo_engine_last_launches)
  phovo_hip::DeviceBuffer<phovo_trust_region_report> tr_reports;   // trust-region objective: the solver records of the enqueue's pairs
  bool tr_ran = false;                         // the enqueue ran under PHOVO_OBJECTIVE_TRUST_REGION
  phovo_hip::DeviceBuffer<double> illum;       // affine-illumination objective: (alpha, beta) of the enqueue's pairs, [pairs][2]
  bool affine_ran = false;                     // the enqueue ran under PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE
  phovo_hip::DeviceBuffer<phovo_geometric_report> geo_reports;     // photometric-geometric objective: the records of the enqueue's pairs
  bool geometric_ran = false;                  // the enqueue ran under PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC
  phovo_hip::DeviceBuffer<phovo_robust_report> rob_reports;        // robust inverse-compositional objective: the records of the enqueue's pairs
  bool robust_ran = false;                     // the enqueue ran under PHOVO_OBJECTIVE_INVERSE_ROBUST
  phovo_hip::DeviceBuffer<phovo_semidense_report> sd_reports;      // semi-dense inverse-compositional objective: the records of the enqueue's pairs
  bool semidense_ran = false;                  // the enqueue ran under PHOVO_OBJECTIVE_INVERSE_SEMIDENSE
  // that objective's pixel lists: [grid][slab] 4-byte records, grid = the persistent grid of the enqueue, slab = the padded
  // size of its largest active level (GNInverseSemiDenseArgs); the slot's own, so two enqueues in flight never share one
  phovo_hip::DeviceBuffer<unsigned> sd_records;
  // phovo_engine_enqueue_align_prior: the enqueue's own prior blocks ([pairs][GN_PRIOR_DOUBLES], copied from the pinned
  // h_prior, which stays untouched until the slot is used again) and the records of its pairs
  phovo_hip::DeviceBuffer<double> prior;
  double *h_prior = nullptr;
  size_t h_prior_capacity = 0;                 // doubles
  phovo_hip::DeviceBuffer<phovo_prior_report> prior_reports;
  bool prior_ran = false;                      // the enqueue carried a prior
  int num_levels = 0;                          // the configuration the enqueue ran under: its levels, and which of them it
  bool level_skipped[PHOVO_MAX_LEVELS] = {};   // skipped (max_num_iterations == 0) -- a fetch may come after a set_config
};

struct phovo_engine {
  int device = 0;
  hipStream_t stream = nullptr;                // uploads, pyramid producers, plane access
  hipStream_t copy_stream = nullptr;           // batched uploads: host-to-device copies of chunk i+1 run beside the pyramid kernels of chunk i
  hipEvent_t ev_copied[2] = {}, ev_built[2] = {};     // per staging half
  // phovo_engine_upload_frames_device: the producer's work so far (recorded on its stream), the last read of its memory
  // and the end of the pyramid build (both recorded on `stream`)
  hipEvent_t ev_ingest_produced = nullptr, ev_ingest_read = nullptr, ev_ingested = nullptr;
  bool ingest_pending = false;                 // `stream` may still be building an ingest's pyramids: enqueues wait for ev_ingested
  phovo_ingest_record last_ingest{};
  AlignSlot slots[PHOVO_ENQUEUE_DEPTH];
  int ticket = 0;                              // tickets handed out so far; enqueue t lives in slots[t % PHOVO_ENQUEUE_DEPTH]

  phovo_config cfg{};
  phovo_extensions ext{};                      // plane storage, Huber deltas: all off by default
  double K[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  bool have_K = false;
  double min_depth = 0.3, max_depth = 5.0;     // ...Analytic.h:430
  bool build_all = false;

  int n_frames = 0, width = 0, height = 0;
  phovo_hip::LevelPool levels[PHOVO_MAX_LEVELS];
  // staging for raw frames: `stage_frames` frames of each kind that has been used so far
  int stage_frames = 0;
  bool stage_has_f64 = false, stage_has_u16 = false;
  uint8_t *d_gray = nullptr;
  double *d_depth = nullptr;
  uint16_t *d_depth16 = nullptr;
  double *d_tmp = nullptr;
  double *d_blur0 = nullptr;                   // blurFilterSize[0] > 0: the blurred level-0 intensity of a staging chunk (see build_pyramids)
  double *d_scratch = nullptr;                 // fp64 planes of one staging chunk (narrow storages, plane get/set)
  double *d_blur_kernel = nullptr;             // [levels][max ksize]
  int blur_kernel_stride = 0;

  int slide_policy = 0;                        // 0 automatic (where the owner map exceeds LDS), -1 never
  int fusion = PHOVO_FUSION_AUTO;              // consecutive levels in one launch (phovo_engine_set_level_fusion)
  int cu_count = 256;
  int wide_policy = 0;                         // 0 auto, 1 always (where possible), -1 never
  bool batch_invariant = false;                // every batch takes the same kernels and geometries (phovo_engine_set_batch_invariant)
  int objective = PHOVO_OBJECTIVE_PHOTOMETRIC;  // phovo_engine_set_objective
  phovo_trust_region_options tr_opt{};         // phovo_engine_set_trust_region_options (Ceres's defaults at creation)
  phovo_geometric_options geo_opt{};           // phovo_engine_set_geometric_options (phovo_geometric_options_default at creation)
  phovo_robust_options rob_opt{};              // phovo_engine_set_robust_options (phovo_robust_options_default at creation)
  phovo_semidense_options sd_opt{};            // phovo_engine_set_semidense_options (phovo_semidense_options_default at creation)
  phovo_prior_options prior_opt{};             // phovo_engine_set_prior_options (phovo_prior_options_default at creation)
  bool latency_forms = false;                  // a handful of pairs may take the forms that finish soonest also where a level has a one-workgroup form with its owner map in LDS (phovo_engine_set_latency_forms)
  std::vector<unsigned char> frame_roles;      // [frame][PHOVO_MAX_LEVELS]: PHOVO_ROLE_* each level of each frame has been given since the
                                               // pool was reserved (an upload: every level; a plane write: its level)
  // The evaluate entry points' own workspace (engine_evaluate.cpp), allocated on first use and kept until the engine is
  // destroyed; phovo_engine_evaluate_pairs keeps its owner maps at the front, and between its calls they hold -1 everywhere
  phovo_hip::DeviceBuffer<unsigned char> eval_ws;
  size_t eval_owner_clean = 0;                 // leading ints of eval_ws known to hold -1
};

namespace phovo_hip {

// Every enqueue in flight has finished when this returns (host wait).  Called by whatever changes device state that a
// running alignment reads: uploads, plane writes, pool and configuration changes.  (engine.cpp)
hipError_t quiesce(phovo_engine *e);

// Everything a slot holds in device and pinned memory goes (engine_align.cpp; the engine's destruction).
void free_slot(AlignSlot &s);

// All refusals of phovo_engine_upload_frames_device that do not depend on the pool; w x h is the frame size the images are
// taken to have.  (engine.cpp; the class surface asks before it drops the pool for a new size)
int ingest_check(const phovo_engine *e, int count, int roles, const phovo_device_image *intensity,
                 const phovo_device_image *depth, double depth_scale, int w, int h);

// The view of one level that GNLevelArgs, GNEvalArgs and GNSampledEvalArgs spell alike: its size, the intrinsics scaled as
// the reference scales them, the depth range and where the planes lie.
template <class Args>
void fill_level_view(Args &a, const phovo_engine *e, int level)
{
  const LevelPool &lv = e->levels[level];
  a.w = lv.w; a.h = lv.h; a.n = lv.n;
  a.n_chunks = (lv.n + 63) / 64;
  const double scaleFactor = 1.0 / std::pow(2, level);                               // ...Analytic.h:203
  a.fx = e->K[0] * scaleFactor; a.fy = e->K[4] * scaleFactor;                        // :204-207
  a.ox = e->K[2] * scaleFactor; a.oy = e->K[5] * scaleFactor;
  a.ifx = 1.f / a.fx; a.ify = 1.f / a.fy;                                            // :208-209
  a.min_depth = e->min_depth; a.max_depth = e->max_depth;
  a.planes = lv.planes;
  a.frame_bytes = lv.frame_bytes;
  for (int p = 0; p < PLANES_PER_FRAME; p++) a.plane_off[p] = lv.plane_off[p];
}

}  // namespace phovo_hip
