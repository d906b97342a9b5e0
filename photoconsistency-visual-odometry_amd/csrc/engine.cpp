// Host side of the C ABI (include/phovo_hip.h), the engine itself: its lifecycle and configuration, the frame pool in HBM,
// uploads, device ingest and plane access.  The alignments are in engine_align.cpp, the systems at given poses in
// engine_evaluate.cpp and the single-pair class surface in odometry_c.cpp (engine_internal.hpp).
// There is no CPU fallback anywhere in these files: without a HIP device every entry point that
// touches data fails with PHOVO_E_HIP.

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "engine_internal.hpp"

namespace phovo_hip {

static thread_local std::string g_last_error;

void set_last_error(const std::string &msg) { g_last_error = msg; }
int fail(int status, const std::string &msg) { g_last_error = msg; return status; }

#ifdef PHOVO_TUNING
bool tuning_switch(const char *name) { return std::getenv(name) != nullptr; }
#endif

hipError_t quiesce(phovo_engine *e)
{
  for (AlignSlot &s : e->slots) {
    if (!s.stream) continue;
    const hipError_t he = hipStreamSynchronize(s.stream);
    if (he != hipSuccess) return he;
  }
  return hipSuccess;
}

}  // namespace phovo_hip

using namespace phovo_hip;

// PHOVO_HIP_CHECK inside an upload: the `drain` in scope first waits out what the upload has put in flight.
#define PHOVO_DRAIN_CHECK(expr)                                                                               \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess) return drain(fail(PHOVO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e))); \
  } while (0)

namespace {

void free_pool(phovo_engine *e)
{
  if (e->ingest_pending && e->stream) (void)hipStreamSynchronize(e->stream);      // a device ingest may still be building
  e->ingest_pending = false;
  for (auto &lv : e->levels) {
    if (lv.planes) (void)hipFree(lv.planes);
    lv = LevelPool{};
  }
  for (void *p : {(void *)e->d_gray, (void *)e->d_depth, (void *)e->d_depth16, (void *)e->d_tmp, (void *)e->d_blur_kernel,
                  (void *)e->d_scratch, (void *)e->d_blur0})
    if (p) (void)hipFree(p);
  e->d_scratch = nullptr; e->d_blur0 = nullptr;
  e->d_gray = nullptr; e->d_depth = nullptr; e->d_depth16 = nullptr; e->d_tmp = nullptr;
  e->d_blur_kernel = nullptr;
  e->stage_frames = 0; e->stage_has_f64 = e->stage_has_u16 = false;
  e->n_frames = 0; e->width = 0; e->height = 0;
  e->frame_roles.clear();
}

// Nothing on the device reads the pool or the configuration any more when this returns (a setter is about to change them).
void settle(phovo_engine *e)
{
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  (void)quiesce(e);
}

// A setter changes what the pool's layout depends on: the pool goes, and reserve_frames and the uploads are the caller's again.
void drop_pool(phovo_engine *e)
{
  settle(e);
  free_pool(e);
}

int validate_config(const phovo_config *c)
{
  if (c->num_levels < 1 || c->num_levels > PHOVO_MAX_LEVELS)
    return fail(PHOVO_E_CONFIG, "num_levels out of range [1, 16]");
  for (int l = 0; l < c->num_levels; l++) {
    if (c->max_num_iterations[l] < 0) return fail(PHOVO_E_CONFIG, "max_num_iterations < 0");
    const int b = c->blur_filter_size[l];
    if (b < 0 || (b > 0 && (b % 2) == 0))
      return fail(PHOVO_E_CONFIG, "blurFilterSize must be 0 or odd (cv::GaussianBlur requires an odd kernel)");
    if (b > 63) return fail(PHOVO_E_CONFIG, "blurFilterSize > 63");
  }
  return PHOVO_OK;
}

void level_dims(int w, int h, int level, int *lw, int *lh)
{
  const double f = 1.0 / (double)(1 << level);        // factor = factor/2  (...Analytic.h:161)
  *lw = (int)std::rint((double)w * f);                // Size(0,0), fx, fy -> cvRound(cols*fx)
  *lh = (int)std::rint((double)h * f);
}

// Every objective but the photometric one runs reference-exact only: fp64 planes, nearest / scatter sampling, no Huber
// weights, jacobian_corrected 0 (the affine-illumination, photometric-geometric and inverse-compositional rows, and the robust
// inverse-compositional objective's own weights, are fixed by the objective, not chosen by the extensions).  PHOVO_OK where `objective` and `x` go together, else the refusal, in the setter's name.
int reference_exact_only(const char *setter, int objective, const phovo_extensions &x)
{
  bool exact = x.plane_storage == PHOVO_STORAGE_F64 && x.sampling == PHOVO_SAMPLING_NEAREST_SCATTER && x.jacobian_corrected == 0;
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++)
    if (x.huber_delta[l] > 0.0) exact = false;
  if (exact || objective == PHOVO_OBJECTIVE_PHOTOMETRIC) return PHOVO_OK;
  const char *only =
      objective == PHOVO_OBJECTIVE_BIOBJECTIVE ? "the bi-objective runs on fp64 planes with nearest / scatter sampling and no Huber weights only"
      : objective == PHOVO_OBJECTIVE_TRUST_REGION ? "the trust-region objective runs on fp64 planes with the default sampling, no Huber weights and jacobian_corrected 0 only"
      : objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE ? "the affine-illumination objective runs on fp64 planes with the default sampling setting, no Huber weights and jacobian_corrected 0 only"
      : objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL ? "the inverse-compositional objective runs on fp64 planes with the default sampling setting, no Huber weights and jacobian_corrected 0 only"
      : objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE ? "the semi-dense inverse-compositional objective runs on fp64 planes with the default sampling setting, no Huber weights and jacobian_corrected 0 only"
      : objective == PHOVO_OBJECTIVE_INVERSE_ROBUST ? "the robust inverse-compositional objective runs on fp64 planes with the default sampling setting, no huber_delta extension and jacobian_corrected 0 only"
      : "the photometric-geometric objective runs on fp64 planes with the default sampling setting, no Huber weights and jacobian_corrected 0 only";
  return fail(PHOVO_E_UNSUPPORTED, std::string(setter) + ": " + only);
}

// Depth gradients (with the max depth in force) and gain of `count` consecutive target frames of level l, from the
// intensity and depth planes already in the pool (fp64, packed: the frame is frame_bytes / 8 doubles).
int build_biobjective_target(phovo_engine *e, int l, int first_frame, int count)
{
  const LevelPool &lv = e->levels[l];
  const double *base = reinterpret_cast<const double *>(lv.planes + (size_t)first_frame * lv.frame_bytes);
  const size_t fstride = lv.frame_bytes / sizeof(double);
  PHOVO_HIP_CHECK(pyr_scharr_scaled(base, fstride, lv.plane_off[PLANE_D] / sizeof(double), lv.dgx_off / sizeof(double),
                                    lv.dgy_off / sizeof(double), count, lv.w, lv.h, 1. / e->max_depth,
                                    e->cfg.image_gradients_scaling_factor[l], e->stream));
  PHOVO_HIP_CHECK(pyr_depth_gain(base, fstride, lv.plane_off[PLANE_I] / sizeof(double), lv.plane_off[PLANE_D] / sizeof(double),
                                 lv.gain_off / sizeof(double), count, lv.n, e->stream));
  return PHOVO_OK;
}

enum DepthKind { DEPTH_NONE = 0, DEPTH_F64 = 1, DEPTH_U16 = 2 };
constexpr int STAGE_CHUNK = 32;      // frames copied and processed per batch of producer launches

// Makes sure the staging buffers hold `frames` raw frames of the kinds asked for.
int ensure_stage(phovo_engine *e, int frames, bool want_f64, bool want_u16)
{
  const size_t px = (size_t)e->width * (size_t)e->height;
  const bool grow = frames > e->stage_frames;
  if (grow || (want_f64 && !e->stage_has_f64) || (want_u16 && !e->stage_has_u16)) {
    PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
    const int cap = grow ? frames : e->stage_frames;
    want_f64 = want_f64 || e->stage_has_f64;
    want_u16 = want_u16 || e->stage_has_u16;
    if (e->d_gray) (void)hipFree(e->d_gray);
    if (e->d_depth) (void)hipFree(e->d_depth);
    if (e->d_depth16) (void)hipFree(e->d_depth16);
    if (e->d_blur0) (void)hipFree(e->d_blur0);
    e->d_gray = nullptr; e->d_depth = nullptr; e->d_depth16 = nullptr; e->d_blur0 = nullptr;
    e->stage_frames = 0; e->stage_has_f64 = e->stage_has_u16 = false;
    PHOVO_HIP_CHECK(hipMalloc(&e->d_gray, px * (size_t)cap));
    // (the blurred level-0 image of ONE chunk: build_pyramids uses it at offset 0 on the engine's stream, whichever
    // staging half the chunk's raw frames sit in)
    if (e->cfg.blur_filter_size[0] > 0)
      PHOVO_HIP_CHECK(hipMalloc(&e->d_blur0, px * (size_t)(cap < STAGE_CHUNK ? cap : STAGE_CHUNK) * sizeof(double)));
    if (want_f64) PHOVO_HIP_CHECK(hipMalloc(&e->d_depth, px * (size_t)cap * sizeof(double)));
    if (want_u16) PHOVO_HIP_CHECK(hipMalloc(&e->d_depth16, px * (size_t)cap * sizeof(uint16_t)));
    e->stage_frames = cap; e->stage_has_f64 = want_f64; e->stage_has_u16 = want_u16;
  }
  return PHOVO_OK;
}

// Builds the pyramids of `count` consecutive frames whose raw data sits in the staging buffers:
// one launch per (level, producer) for the whole batch.
int build_pyramids(phovo_engine *e, int first_frame, int count, int roles, DepthKind kind, double depth_scale,
                   int stage_offset = 0)
{
  const int w = e->width, h = e->height;
  const size_t px = (size_t)w * (size_t)h;
  // the raw frames of this chunk sit `stage_offset` frames into the staging buffers (double-buffered uploads)
  const uint8_t *s_gray = e->d_gray + px * (size_t)stage_offset;
  const double *s_depth = e->d_depth ? e->d_depth + px * (size_t)stage_offset : nullptr;
  const uint16_t *s_depth16 = e->d_depth16 ? e->d_depth16 + px * (size_t)stage_offset : nullptr;
  const int storage = e->ext.plane_storage;
  // blurFilterSize[0] > 0: the converted level-0 image, blurred twice, is the image every other level is resized from
  // (whether or not level 0 itself is resident)
  const double *blurred0 = nullptr;
  if (e->cfg.blur_filter_size[0] > 0) {
    const int ks0 = e->cfg.blur_filter_size[0];
    PHOVO_HIP_CHECK(pyr_intensity_level(s_gray, px, count, w, h, 0, w, h, e->d_blur0, px, e->stream));   // convertTo  :471,484
    for (int f = 0; f < count; f++) {
      PHOVO_HIP_CHECK(pyr_gaussian_blur(e->d_blur0 + (size_t)f * px, e->d_tmp, w, h, ks0, e->d_blur_kernel, e->stream));
      PHOVO_HIP_CHECK(pyr_gaussian_blur(e->d_blur0 + (size_t)f * px, e->d_tmp, w, h, ks0, e->d_blur_kernel, e->stream));
    }
    blurred0 = e->d_blur0;
  }
  for (int l = 0; l < e->cfg.num_levels; l++) {
    LevelPool &lv = e->levels[l];
    if (!lv.stored) continue;
    // fp64 storage: the producers write straight into the pool.  Narrow storage: they write fp64 planes into
    // the scratch chunk (same [frame][4][n] layout) and a convert pass rounds them into the pool once.
    const bool direct = storage == PHOVO_STORAGE_F64 && lv.rec_off == 0;
    // (fp64, packed: the frame as the pool holds it -- four planes, and under the bi-objective the target planes behind them)
    const size_t fstride = direct ? lv.frame_bytes / sizeof(double) : (size_t)PLANES_PER_FRAME * (size_t)lv.n;
    double *base = direct ? reinterpret_cast<double *>(lv.planes + (size_t)first_frame * lv.frame_bytes) : e->d_scratch;
    // BuildPyramid(intensity, applyBlur = true)  :474,487
    const int ks = e->cfg.blur_filter_size[l];
    const double *kern = ks > 0 ? e->d_blur_kernel + (size_t)l * e->blur_kernel_stride : nullptr;
    if (blurred0) {
      // Level 0 was blurred IN PLACE (`imgAux = img` is a shallow cv::Mat alias, :136, and GaussianBlur(imgAux, imgAux)
      // writes through it, :146-147), so every cv::resize(img, ...) of the later levels (:132) reads the blurred
      // level 0 (blurred0, made before this loop); level 0 itself is that image, not blurred a second time.
      PHOVO_HIP_CHECK(pyr_depth_level(blurred0, px, count, w, h, l, lv.w, lv.h, base + (size_t)PLANE_I * lv.n, fstride,
                                      e->stream));
    } else {
      PHOVO_HIP_CHECK(pyr_intensity_level(s_gray, px, count, w, h, l, lv.w, lv.h,
                                          base + (size_t)PLANE_I * lv.n, fstride, e->stream));
    }
    if (ks > 0 && !(blurred0 && l == 0)) {                              // GaussianBlur twice  :144-148
      for (int f = 0; f < count; f++) {
        double *pi = base + (size_t)f * fstride + (size_t)PLANE_I * lv.n;
        PHOVO_HIP_CHECK(pyr_gaussian_blur(pi, e->d_tmp, lv.w, lv.h, ks, kern, e->stream));
        PHOVO_HIP_CHECK(pyr_gaussian_blur(pi, e->d_tmp, lv.w, lv.h, ks, kern, e->stream));
      }
    }
    const bool bi_target = e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE && (roles & PHOVO_ROLE_TARGET);
    if ((roles & PHOVO_ROLE_SOURCE) || bi_target) {                     // BuildPyramid(depth, false)  :475 (...BiObjective.h:573)
      double *pd = base + (size_t)PLANE_D * lv.n;
      if (kind == DEPTH_U16)
        PHOVO_HIP_CHECK(pyr_depth_level_u16(s_depth16, px, depth_scale, count, w, h, l, lv.w, lv.h, pd, fstride, e->stream));
      else
        PHOVO_HIP_CHECK(pyr_depth_level(s_depth, px, count, w, h, l, lv.w, lv.h, pd, fstride, e->stream));
    }
    if (roles & PHOVO_ROLE_TARGET)                                      // BuildDerivativesPyramids  :490
      PHOVO_HIP_CHECK(pyr_scharr(base, fstride, (size_t)PLANE_I * lv.n, (size_t)PLANE_GX * lv.n,
                                 (size_t)PLANE_GY * lv.n, count, lv.w, lv.h,
                                 e->cfg.image_gradients_scaling_factor[l], e->stream));
    if (!direct) {
      unsigned char *dst = lv.planes + (size_t)first_frame * lv.frame_bytes;
      const bool want[PLANES_PER_FRAME] = {true, (roles & PHOVO_ROLE_SOURCE) != 0, (roles & PHOVO_ROLE_TARGET) != 0,
                                           (roles & PHOVO_ROLE_TARGET) != 0};
      for (int p = 0; p < PLANES_PER_FRAME; p++) {
        if (!want[p]) continue;
        PHOVO_HIP_CHECK(pyr_store_plane(base + (size_t)p * lv.n, fstride, count, lv.n, dst + lv.plane_off[p],
                                        lv.frame_bytes, storage, p == PLANE_D, e->stream));
      }
    }
    if (lv.rec_off && (roles & PHOVO_ROLE_TARGET))                      // bilinear sampling: the target's tap records
      PHOVO_HIP_CHECK(pyr_build_tap_records(lv.planes + (size_t)first_frame * lv.frame_bytes, lv.frame_bytes, lv.plane_off,
                                            lv.rec_off, count, lv.n, storage, e->stream));
    if (bi_target) {                                                    // BuildDepthDerivativesPyramids  :577, gain  :300
      const int st = build_biobjective_target(e, l, first_frame, count);
      if (st != PHOVO_OK) return st;
    }
  }
  return PHOVO_OK;
}

int copy_rows_to_device(void *dst, const void *src, size_t stride, size_t row_bytes, int rows,
                        hipStream_t stream)
{
  if (stride == row_bytes) {
    PHOVO_HIP_CHECK(hipMemcpyAsync(dst, src, row_bytes * (size_t)rows, hipMemcpyHostToDevice, stream));
  } else {
    if (stride < row_bytes) return fail(PHOVO_E_INVALID_ARGUMENT, "stride smaller than a row");
    PHOVO_HIP_CHECK(hipMemcpy2DAsync(dst, row_bytes, src, stride, row_bytes, (size_t)rows,
                                     hipMemcpyHostToDevice, stream));
  }
  return PHOVO_OK;
}

}  // namespace

extern "C" {

const char *phovo_version(void) { return "phovo-hip 0.1.0 (gfx950)"; }

const char *phovo_status_string(int status)
{
  switch (status) {
    case PHOVO_OK: return "ok";
    case PHOVO_E_INVALID_ARGUMENT: return "invalid argument";
    case PHOVO_E_CONFIG: return "configuration error";
    case PHOVO_E_SHAPE: return "shape error";
    case PHOVO_E_HIP: return "HIP runtime error";
    case PHOVO_E_NOT_READY: return "not ready (call order)";
    case PHOVO_E_IO: return "I/O error";
    case PHOVO_E_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
  }
}

const char *phovo_last_error(void) { return g_last_error.c_str(); }

int phovo_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int phovo_config_default(phovo_config *cfg)
{
  if (!cfg) return fail(PHOVO_E_INVALID_ARGUMENT, "phovo_config_default: null");
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->num_levels = 5;                                   // ...Analytic.h:433
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++) {
    cfg->blur_filter_size[l] = 0;                        // :434
    cfg->image_gradients_scaling_factor[l] = 0.0625;     // :435
    cfg->lambda_optimization_step[l] = 1.0;              // :436
    cfg->max_num_iterations[l] = 0;                      // :437
    cfg->min_gradient_norm[l] = 300.0;                   // :441
  }
  cfg->max_num_iterations[2] = 5;                        // :438
  cfg->max_num_iterations[3] = 20;                       // :439
  cfg->max_num_iterations[4] = 50;                       // :440
  cfg->visualize_iterations = 0;                         // :442
  return PHOVO_OK;
}

int phovo_config_read_file(const char *path, phovo_config *cfg) { return read_config_file(path, cfg); }

int phovo_eigen_pose(const double s[6], double rt[16])
{
  if (!s || !rt) return fail(PHOVO_E_INVALID_ARGUMENT, "phovo_eigen_pose: null");
  const double x = s[0], y = s[1], z = s[2], yaw = s[3], pitch = s[4], roll = s[5];
  rt[0] = std::cos(yaw) * std::cos(pitch);               // CPhotoconsistencyOdometry.h:52-70
  rt[1] = std::cos(yaw) * std::sin(pitch) * std::sin(roll) - std::sin(yaw) * std::cos(roll);
  rt[2] = std::cos(yaw) * std::sin(pitch) * std::cos(roll) + std::sin(yaw) * std::sin(roll);
  rt[3] = x;
  rt[4] = std::sin(yaw) * std::cos(pitch);
  rt[5] = std::sin(yaw) * std::sin(pitch) * std::sin(roll) + std::cos(yaw) * std::cos(roll);
  rt[6] = std::sin(yaw) * std::sin(pitch) * std::cos(roll) - std::cos(yaw) * std::sin(roll);
  rt[7] = y;
  rt[8] = -std::sin(pitch);
  rt[9] = std::cos(pitch) * std::sin(roll);
  rt[10] = std::cos(pitch) * std::cos(roll);
  rt[11] = z;
  rt[12] = 0; rt[13] = 0; rt[14] = 0; rt[15] = 1;
  return PHOVO_OK;
}

int phovo_state_from_pose(const double rt[16], double s[6])
{
  if (!rt || !s) return fail(PHOVO_E_INVALID_ARGUMENT, "phovo_state_from_pose: null");
  s[0] = rt[3]; s[1] = rt[7]; s[2] = rt[11];
  s[3] = std::atan2(rt[4], rt[0]);
  s[4] = std::atan2(-rt[8], std::sqrt(rt[0] * rt[0] + rt[4] * rt[4]));
  s[5] = std::atan2(rt[9], rt[10]);
  return PHOVO_OK;
}

/* ------------------------------------------------------------------ engine ------------------ */

int phovo_engine_create(int device, phovo_engine **out)
{
  if (!out) return fail(PHOVO_E_INVALID_ARGUMENT, "phovo_engine_create: null");
  *out = nullptr;
  int count = 0;
  hipError_t err = hipGetDeviceCount(&count);
  if (err != hipSuccess || count <= 0)
    return fail(PHOVO_E_HIP, "no HIP device available: this library has no CPU path");
  if (device < 0 || device >= count) return fail(PHOVO_E_INVALID_ARGUMENT, "device index out of range");
  PHOVO_HIP_CHECK(hipSetDevice(device));
  phovo_engine *e = new (std::nothrow) phovo_engine();
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "out of host memory");
  e->device = device;
  phovo_config_default(&e->cfg);
  phovo_extensions_default(&e->ext);
  phovo_trust_region_options_default(&e->tr_opt);
  phovo_geometric_options_default(&e->geo_opt);
  phovo_robust_options_default(&e->rob_opt);
  phovo_semidense_options_default(&e->sd_opt);
  phovo_prior_options_default(&e->prior_opt);
  hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
  if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking);
  for (int i = 0; i < 2 && he == hipSuccess; i++) {
    he = hipEventCreateWithFlags(&e->ev_copied[i], hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_built[i], hipEventDisableTiming);
  }
  for (hipEvent_t *ev : {&e->ev_ingest_produced, &e->ev_ingest_read, &e->ev_ingested})
    if (he == hipSuccess) he = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  for (AlignSlot &s : e->slots) {
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipEventCreate(&s.ev_total_start);
    if (he == hipSuccess) he = hipEventCreate(&s.ev_total_stop);
    for (int l = 0; l < PHOVO_MAX_LEVELS && he == hipSuccess; l++) {
      he = hipEventCreate(&s.ev_start[l]);
      if (he == hipSuccess) he = hipEventCreate(&s.ev_stop[l]);
    }
  }
  if (he == hipSuccess) he = gn_prepare_kernels();
  if (he == hipSuccess) he = gn_prepare_slide_kernels();
  if (he == hipSuccess) he = gn_prepare_biobjective_kernels();
  if (he == hipSuccess) he = gn_prepare_trust_region_kernels();
  if (he == hipSuccess) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) e->cu_count = cus;
  }
  if (he != hipSuccess) {
    phovo_engine_destroy(e);
    return fail(PHOVO_E_HIP, std::string("engine setup: ") + hipGetErrorString(he));
  }
  *out = e;
  return PHOVO_OK;
}

int phovo_engine_destroy(phovo_engine *e)
{
  if (!e) return PHOVO_OK;
  (void)hipSetDevice(e->device);
  if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  (void)quiesce(e);
  free_pool(e);
  e->eval_ws.release();
  for (AlignSlot &s : e->slots) {
    free_slot(s);
    for (int l = 0; l < PHOVO_MAX_LEVELS; l++) {
      if (s.ev_start[l]) (void)hipEventDestroy(s.ev_start[l]);
      if (s.ev_stop[l]) (void)hipEventDestroy(s.ev_stop[l]);
    }
    if (s.ev_total_start) (void)hipEventDestroy(s.ev_total_start);
    if (s.ev_total_stop) (void)hipEventDestroy(s.ev_total_stop);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  for (int i = 0; i < 2; i++) {
    if (e->ev_copied[i]) (void)hipEventDestroy(e->ev_copied[i]);
    if (e->ev_built[i]) (void)hipEventDestroy(e->ev_built[i]);
  }
  for (hipEvent_t ev : {e->ev_ingest_produced, e->ev_ingest_read, e->ev_ingested})
    if (ev) (void)hipEventDestroy(ev);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return PHOVO_OK;
}

int phovo_engine_set_config(phovo_engine *e, const phovo_config *cfg)
{
  if (!e || !cfg) return fail(PHOVO_E_INVALID_ARGUMENT, "set_config: null");
  const int st = validate_config(cfg);
  if (st != PHOVO_OK) return st;
  // A configuration that changes which levels exist or how their planes are built drops the pool:
  // the reference requires the configuration before Set*Frame (:474 uses m_NumOptimizationLevels).
  // Changing only lambda / max_num_iterations (within the resident levels) / min_gradient_norm keeps it.
  bool keep = e->n_frames > 0 && cfg->num_levels == e->cfg.num_levels;
  for (int l = 0; keep && l < cfg->num_levels; l++) {
    if (cfg->blur_filter_size[l] != e->cfg.blur_filter_size[l]) keep = false;
    if (cfg->image_gradients_scaling_factor[l] != e->cfg.image_gradients_scaling_factor[l]) keep = false;
    if (cfg->max_num_iterations[l] > 0 && !e->levels[l].stored) keep = false;
  }
  settle(e);
  if (!keep) free_pool(e);
  e->cfg = *cfg;
  return PHOVO_OK;
}

int phovo_extensions_default(phovo_extensions *ext)
{
  if (!ext) return fail(PHOVO_E_INVALID_ARGUMENT, "phovo_extensions_default: null");
  std::memset(ext, 0, sizeof(*ext));
  ext->plane_storage = PHOVO_STORAGE_F64;
  return PHOVO_OK;
}

int phovo_extensions_read_file(const char *path, phovo_extensions *ext) { return read_extensions_file(path, ext); }

int phovo_engine_set_extensions(phovo_engine *e, const phovo_extensions *ext)
{
  if (!e || !ext) return fail(PHOVO_E_INVALID_ARGUMENT, "set_extensions: null");
  if (ext->plane_storage != PHOVO_STORAGE_F64 && ext->plane_storage != PHOVO_STORAGE_F32 &&
      ext->plane_storage != PHOVO_STORAGE_F16)
    return fail(PHOVO_E_INVALID_ARGUMENT, "set_extensions: unknown plane_storage");
  if (ext->sampling != PHOVO_SAMPLING_NEAREST_SCATTER && ext->sampling != PHOVO_SAMPLING_BILINEAR)
    return fail(PHOVO_E_INVALID_ARGUMENT, "set_extensions: unknown sampling");
  if (ext->jacobian_corrected != 0 && ext->sampling != PHOVO_SAMPLING_BILINEAR)
    return fail(PHOVO_E_UNSUPPORTED, "set_extensions: jacobian_corrected needs sampling = PHOVO_SAMPLING_BILINEAR "
                                     "(the scatter path is kept reference-exact)");
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++)
    if (!(ext->huber_delta[l] == ext->huber_delta[l])) return fail(PHOVO_E_INVALID_ARGUMENT, "set_extensions: huber_delta is NaN");
  const int st = reference_exact_only("set_extensions", e->objective, *ext);
  if (st != PHOVO_OK) return st;
  // the pool layout changes with the storage type, and -- fp16 planes under bilinear sampling carry tap records -- with the
  // sampling where that adds or removes the records
  auto has_records = [](const phovo_extensions &x) { return x.sampling == PHOVO_SAMPLING_BILINEAR && x.plane_storage == PHOVO_STORAGE_F16; };
  if (ext->plane_storage != e->ext.plane_storage || has_records(*ext) != has_records(e->ext)) drop_pool(e);
  e->ext = *ext;
  return PHOVO_OK;
}

int phovo_engine_set_objective(phovo_engine *e, int objective)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_objective: null");
  if (objective != PHOVO_OBJECTIVE_PHOTOMETRIC && objective != PHOVO_OBJECTIVE_BIOBJECTIVE &&
      objective != PHOVO_OBJECTIVE_TRUST_REGION && objective != PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE &&
      objective != PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC && objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL &&
      objective != PHOVO_OBJECTIVE_INVERSE_ROBUST && objective != PHOVO_OBJECTIVE_INVERSE_SEMIDENSE)
    return fail(PHOVO_E_INVALID_ARGUMENT, "set_objective: unknown objective");
  const int st = reference_exact_only("set_objective", objective, e->ext);
  if (st != PHOVO_OK) return st;
  // The photometric, trust-region, affine-illumination, photometric-geometric and the three inverse-compositional objectives share
  // the frame layout: a switch between them keeps the pool.
  auto bi = [](int o) { return o == PHOVO_OBJECTIVE_BIOBJECTIVE; };
  if (objective != e->objective && (bi(objective) || bi(e->objective))) drop_pool(e);   // the pool layout changes (the bi-objective's target planes)
  e->objective = objective;
  return PHOVO_OK;
}

int phovo_engine_get_objective(const phovo_engine *e, int *objective)
{
  if (!e || !objective) return fail(PHOVO_E_INVALID_ARGUMENT, "get_objective: null");
  *objective = e->objective;
  return PHOVO_OK;
}

int phovo_trust_region_read_file(const char *path, phovo_config *cfg, phovo_trust_region_options *opt)
{
  return read_trust_region_file(path, cfg, opt);
}

int phovo_engine_set_trust_region_options(phovo_engine *e, const phovo_trust_region_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "set_trust_region_options: null");
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++) {
    const double v[7] = {opt->function_tolerance[l], opt->gradient_tolerance[l], opt->parameter_tolerance[l],
                         opt->initial_trust_region_radius[l], opt->max_trust_region_radius[l],
                         opt->min_trust_region_radius[l], opt->min_relative_decrease[l]};
    for (double x : v)
      if (!(x == x)) return fail(PHOVO_E_INVALID_ARGUMENT, "set_trust_region_options: NaN");
    if (!(opt->initial_trust_region_radius[l] > 0.0))
      return fail(PHOVO_E_INVALID_ARGUMENT, "set_trust_region_options: initial_trust_region_radius must be positive");
  }
  e->tr_opt = *opt;
  return PHOVO_OK;
}

int phovo_engine_get_trust_region_options(const phovo_engine *e, phovo_trust_region_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "get_trust_region_options: null");
  *opt = e->tr_opt;
  return PHOVO_OK;
}

int phovo_geometric_read_file(const char *path, phovo_geometric_options *opt) { return read_geometric_file(path, opt); }

int phovo_engine_set_geometric_options(phovo_engine *e, const phovo_geometric_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "set_geometric_options: null");
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++)
    if (!(opt->depth_weight[l] > 0.0 && std::isfinite(opt->depth_weight[l])))
      return fail(PHOVO_E_INVALID_ARGUMENT, "set_geometric_options: every depth_weight must be finite and > 0");
  e->geo_opt = *opt;
  return PHOVO_OK;
}

int phovo_engine_get_geometric_options(const phovo_engine *e, phovo_geometric_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "get_geometric_options: null");
  *opt = e->geo_opt;
  return PHOVO_OK;
}

int phovo_robust_options_default(phovo_robust_options *opt)
{
  if (!opt) return fail(PHOVO_E_INVALID_ARGUMENT, "robust_options_default: null");
  opt->scale_factor = 1.345 * 1.4826;
  return PHOVO_OK;
}

int phovo_engine_set_robust_options(phovo_engine *e, const phovo_robust_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "set_robust_options: null");
  if (!(opt->scale_factor > 0.0 && std::isfinite(opt->scale_factor)))
    return fail(PHOVO_E_INVALID_ARGUMENT, "set_robust_options: scale_factor must be finite and > 0");
  e->rob_opt = *opt;
  return PHOVO_OK;
}

int phovo_engine_get_robust_options(const phovo_engine *e, phovo_robust_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "get_robust_options: null");
  *opt = e->rob_opt;
  return PHOVO_OK;
}

int phovo_semidense_read_file(const char *path, phovo_semidense_options *opt) { return read_semidense_file(path, opt); }

int phovo_engine_set_semidense_options(phovo_engine *e, const phovo_semidense_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "set_semidense_options: null");
  for (double t : opt->min_pixel_gradient)
    if (!(t >= 0.0 && std::isfinite(t)))
      return fail(PHOVO_E_INVALID_ARGUMENT, "set_semidense_options: every min_pixel_gradient must be finite and >= 0");
  e->sd_opt = *opt;
  return PHOVO_OK;
}

int phovo_engine_get_semidense_options(const phovo_engine *e, phovo_semidense_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "get_semidense_options: null");
  *opt = e->sd_opt;
  return PHOVO_OK;
}

int phovo_prior_options_default(phovo_prior_options *opt)
{
  if (!opt) return fail(PHOVO_E_INVALID_ARGUMENT, "prior_options_default: null");
  for (double &s : opt->level_scale) s = 1.0;
  return PHOVO_OK;
}

int phovo_engine_set_prior_options(phovo_engine *e, const phovo_prior_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "set_prior_options: null");
  for (double s : opt->level_scale)
    if (!(s >= 0.0 && std::isfinite(s)))
      return fail(PHOVO_E_INVALID_ARGUMENT, "set_prior_options: every level_scale must be finite and >= 0");
  e->prior_opt = *opt;
  return PHOVO_OK;
}

int phovo_engine_get_prior_options(const phovo_engine *e, phovo_prior_options *opt)
{
  if (!e || !opt) return fail(PHOVO_E_INVALID_ARGUMENT, "get_prior_options: null");
  *opt = e->prior_opt;
  return PHOVO_OK;
}

int phovo_engine_get_extensions(const phovo_engine *e, phovo_extensions *ext)
{
  if (!e || !ext) return fail(PHOVO_E_INVALID_ARGUMENT, "get_extensions: null");
  *ext = e->ext;
  return PHOVO_OK;
}

int phovo_engine_get_config(const phovo_engine *e, phovo_config *cfg)
{
  if (!e || !cfg) return fail(PHOVO_E_INVALID_ARGUMENT, "get_config: null");
  *cfg = e->cfg;
  return PHOVO_OK;
}

int phovo_engine_set_intrinsic_matrix(phovo_engine *e, const double k[9])
{
  if (!e || !k) return fail(PHOVO_E_INVALID_ARGUMENT, "set_intrinsic_matrix: null");
  std::memcpy(e->K, k, sizeof(e->K));
  e->have_K = true;
  return PHOVO_OK;
}

int phovo_engine_set_depth_range(phovo_engine *e, double min_depth, double max_depth)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_depth_range: null");
  e->min_depth = min_depth;
  e->max_depth = max_depth;
  return PHOVO_OK;
}

int phovo_engine_set_wide_policy(phovo_engine *e, int policy)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_wide_policy: null");
  if (policy < -1 || policy > 1) return fail(PHOVO_E_INVALID_ARGUMENT, "set_wide_policy: policy must be -1, 0 or 1");
  e->wide_policy = policy;
  return PHOVO_OK;
}

int phovo_engine_set_slide_policy(phovo_engine *e, int policy)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_slide_policy: null");
  if (policy < -1 || policy > 0) return fail(PHOVO_E_INVALID_ARGUMENT, "set_slide_policy: policy must be -1 or 0");
  e->slide_policy = policy;
  return PHOVO_OK;
}

int phovo_engine_set_level_fusion(phovo_engine *e, int mode)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_level_fusion: null");
  if (mode != PHOVO_FUSION_AUTO && mode != PHOVO_FUSION_OFF && mode != PHOVO_FUSION_SPLIT)
    return fail(PHOVO_E_INVALID_ARGUMENT, "set_level_fusion: unknown mode");
  e->fusion = mode;
  return PHOVO_OK;
}

int phovo_engine_set_latency_forms(phovo_engine *e, int on)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_latency_forms: null");
  e->latency_forms = on != 0;
  return PHOVO_OK;
}

int phovo_engine_set_batch_invariant(phovo_engine *e, int on)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_batch_invariant: null");
  e->batch_invariant = on != 0;
  return PHOVO_OK;
}

int phovo_engine_set_build_all_levels(phovo_engine *e, int on)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "set_build_all_levels: null");
  if ((on != 0) != e->build_all) drop_pool(e);
  e->build_all = on != 0;
  return PHOVO_OK;
}

// The ranges this library has page-locked, by start address.  The contract of the two entry points is the library's,
// not the runtime's (which, depending on its version, accepts a second registration of a range or an unregister of a
// pointer it never saw without saying so): a range that overlaps a registered one is refused, and so is an unregister
// of anything but the start of a registered range.
static std::mutex g_registry_mutex;
static std::map<uintptr_t, size_t> g_registry;

int phovo_host_register(void *ptr, size_t bytes)
{
  if (!ptr || bytes == 0) return fail(PHOVO_E_INVALID_ARGUMENT, "host_register: null or empty");
  const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
  if (a + bytes < a) return fail(PHOVO_E_INVALID_ARGUMENT, "host_register: the range wraps around the address space");
  std::lock_guard<std::mutex> lock(g_registry_mutex);
  auto next = g_registry.lower_bound(a);                    // first registered range starting at or behind `a`
  if (next != g_registry.end() && next->first < a + bytes)
    return fail(PHOVO_E_INVALID_ARGUMENT, "host_register: the range overlaps one that is already registered");
  if (next != g_registry.begin()) {
    auto prev = std::prev(next);
    if (prev->first + prev->second > a)
      return fail(PHOVO_E_INVALID_ARGUMENT, "host_register: the range overlaps one that is already registered");
  }
  PHOVO_HIP_CHECK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  g_registry[a] = bytes;
  return PHOVO_OK;
}

int phovo_host_unregister(void *ptr)
{
  if (!ptr) return fail(PHOVO_E_INVALID_ARGUMENT, "host_unregister: null");
  std::lock_guard<std::mutex> lock(g_registry_mutex);
  auto it = g_registry.find(reinterpret_cast<uintptr_t>(ptr));
  if (it == g_registry.end())
    return fail(PHOVO_E_INVALID_ARGUMENT, "host_unregister: not the start of a range registered with phovo_host_register");
  PHOVO_HIP_CHECK(hipHostUnregister(ptr));
  g_registry.erase(it);
  return PHOVO_OK;
}

int phovo_engine_reserve_frames(phovo_engine *e, int n_frames, int width, int height)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "reserve_frames: null");
  if (n_frames < 1 || width < 1 || height < 1) return fail(PHOVO_E_INVALID_ARGUMENT, "reserve_frames: sizes must be positive");
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  PHOVO_HIP_CHECK(quiesce(e));
  free_pool(e);
  size_t max_n = 0;
  int max_ks = 0;
  for (int l = 0; l < e->cfg.num_levels; l++) {
    LevelPool &lv = e->levels[l];
    level_dims(width, height, l, &lv.w, &lv.h);
    if (lv.w < 1 || lv.h < 1) { free_pool(e); return fail(PHOVO_E_SHAPE, "image too small for the number of pyramid levels"); }
    lv.n = lv.w * lv.h;
    lv.stored = e->build_all || e->cfg.max_num_iterations[l] > 0;
    const bool fp64_planes = e->ext.plane_storage == PHOVO_STORAGE_F64;
    lv.plan_ok = gn_plan_level(lv.n, &lv.plan, 0, fp64_planes);
    lv.plan_few_ok = gn_plan_level(lv.n, &lv.plan_few, 1, fp64_planes);
    {   // byte layout of one frame at this level: planes I, D, GX, GY.  fp64: packed [4][n] doubles, which is
        // what the producer kernels write directly; narrow storages: every plane starts 16-byte aligned.
      // Bilinear sampling (extension): behind the planes every frame carries its tap records (pyr_build_tap_records), so
      // the frame is no longer what the producers write in one piece.
      const bool records = e->ext.sampling == PHOVO_SAMPLING_BILINEAR && e->ext.plane_storage == PHOVO_STORAGE_F16;      // (fp16 planes only: gn_bilinear_kernel.hip)
      const bool packed = e->ext.plane_storage == PHOVO_STORAGE_F64 && !records;
      size_t off = 0;
      for (int p = 0; p < PLANES_PER_FRAME; p++) {
        lv.plane_off[p] = off;
        const size_t bytes = storage_elem_size(e->ext.plane_storage, p == PLANE_D) * (size_t)lv.n;
        off += packed ? bytes : ((bytes + 15) & ~(size_t)15);
      }
      lv.rec_off = 0;
      if (records) {
        off = (off + 31) & ~(size_t)31;
        lv.rec_off = off;
        off += 4 * storage_elem_size(e->ext.plane_storage, false) * (size_t)lv.n;
        off = (off + 31) & ~(size_t)31;
      }
      lv.dgx_off = lv.dgy_off = lv.gain_off = 0;
      lv.plan_bi_ok = false;
      if (e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE) {     // (fp64 packed planes only: biobjective_supports)
        lv.dgx_off = off;
        lv.dgy_off = off + sizeof(double) * (size_t)lv.n;
        lv.gain_off = off + 2 * sizeof(double) * (size_t)lv.n;
        // (frames start on a 128-byte line, as the packed fp64 layout's 32n bytes do for every level of 4+ pixels: a wave's
        // 512-byte plane load then touches 4 lines, not 5)
        off = (lv.gain_off + sizeof(double) + 127) & ~(size_t)127;
        lv.plan_bi_ok = gn_plan_level_biobjective(lv.n, &lv.plan_bi);
      }
      lv.frame_bytes = off;
      lv.plan_tr_ok = gn_plan_level_trust_region(lv.n, &lv.plan_tr);
    }
    if (lv.stored) {
      const size_t bytes = (size_t)n_frames * lv.frame_bytes;
      hipError_t he = hipMalloc(&lv.planes, bytes);
      if (he != hipSuccess) { free_pool(e); return fail(PHOVO_E_HIP, std::string("hipMalloc(frame pool): ") + hipGetErrorString(he)); }
      he = hipMemsetAsync(lv.planes, 0, bytes, e->stream);
      if (he != hipSuccess) { free_pool(e); return fail(PHOVO_E_HIP, std::string("hipMemset(frame pool): ") + hipGetErrorString(he)); }
      if ((size_t)lv.n > max_n) max_n = (size_t)lv.n;
    }
    if (e->cfg.blur_filter_size[l] > max_ks) max_ks = e->cfg.blur_filter_size[l];
  }
  hipError_t he = hipSuccess;        // raw-frame staging is allocated on first upload (ensure_stage)
  {   // fp64 scratch: one staging chunk of planes for the narrow storages, one frame for plane get/set otherwise
    const size_t frames = e->ext.plane_storage == PHOVO_STORAGE_F64 ? 1 : (size_t)STAGE_CHUNK;
    he = hipMalloc(&e->d_scratch, sizeof(double) * frames * PLANES_PER_FRAME * (max_n ? max_n : 1));
  }
  if (he == hipSuccess && max_ks > 0) {
    // (a level-0 blur runs at full resolution even when level 0 is not resident)
    const size_t tmp_n = e->cfg.blur_filter_size[0] > 0 ? (size_t)width * (size_t)height : max_n;
    he = hipMalloc(&e->d_tmp, sizeof(double) * (tmp_n ? tmp_n : 1));
    if (he == hipSuccess) he = hipMalloc(&e->d_blur_kernel, sizeof(double) * (size_t)max_ks * PHOVO_MAX_LEVELS);
    if (he == hipSuccess) {
      // getGaussianKernel(k, sigma = 3, CV_64F): exp(-0.5/sigma^2 * (i-(k-1)/2)^2), normalised.
      e->blur_kernel_stride = max_ks;
      std::vector<double> kern((size_t)max_ks * PHOVO_MAX_LEVELS, 0.0);
      for (int l = 0; l < e->cfg.num_levels; l++) {
        const int ks = e->cfg.blur_filter_size[l];
        if (ks <= 0) continue;
        const double sigma = 3.0, scale2x = -0.5 / (sigma * sigma);
        double sum = 0;
        double *kk = kern.data() + (size_t)l * max_ks;
        for (int i = 0; i < ks; i++) {
          const double x = i - (ks - 1) * 0.5;
          const double t = std::exp(scale2x * x * x);
          kk[i] = t; sum += t;
        }
        sum = 1. / sum;
        for (int i = 0; i < ks; i++) kk[i] *= sum;
      }
      he = hipMemcpy(e->d_blur_kernel, kern.data(), sizeof(double) * kern.size(), hipMemcpyHostToDevice);
    }
  }
  if (he != hipSuccess) { free_pool(e); return fail(PHOVO_E_HIP, std::string("hipMalloc(staging): ") + hipGetErrorString(he)); }
  e->n_frames = n_frames; e->width = width; e->height = height;
  e->frame_roles.assign((size_t)n_frames * PHOVO_MAX_LEVELS, 0);
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  return PHOVO_OK;
}

int phovo_engine_level_size(const phovo_engine *e, int level, int *width, int *height)
{
  if (!e || !width || !height) return fail(PHOVO_E_INVALID_ARGUMENT, "level_size: null");
  if (level < 0 || level >= e->cfg.num_levels) return fail(PHOVO_E_INVALID_ARGUMENT, "level out of range");
  if (e->n_frames == 0) return fail(PHOVO_E_NOT_READY, "no frame pool reserved");
  *width = e->levels[level].w;
  *height = e->levels[level].h;
  return PHOVO_OK;
}

int phovo_engine_level_is_stored(const phovo_engine *e, int level)
{
  if (!e || level < 0 || level >= e->cfg.num_levels || e->n_frames == 0) return 0;
  return e->levels[level].stored ? 1 : 0;
}

// Copies `count` frames (rows `stride` bytes apart, frames `frame_stride` bytes apart) into a packed
// staging buffer.
static int stage_frames_h2d(phovo_engine *e, void *dst, const void *src, size_t stride, size_t frame_stride,
                            size_t elem, int count, hipStream_t stream)
{
  const size_t row = elem * (size_t)e->width, frame_bytes = row * (size_t)e->height;
  if (stride == row && (frame_stride == frame_bytes || count == 1)) {
    PHOVO_HIP_CHECK(hipMemcpyAsync(dst, src, frame_bytes * (size_t)count, hipMemcpyHostToDevice, stream));
    return PHOVO_OK;
  }
  for (int f = 0; f < count; f++) {
    const int st = copy_rows_to_device(static_cast<char *>(dst) + frame_bytes * (size_t)f,
                                       static_cast<const char *>(src) + frame_stride * (size_t)f, stride, row,
                                       e->height, stream);
    if (st != PHOVO_OK) return st;
  }
  return PHOVO_OK;
}

static int upload_batch(phovo_engine *e, int first_frame, int count, int roles,
                        const uint8_t *intensity, size_t istride, size_t iframe_stride,
                        const void *depth, size_t dstride, size_t dframe_stride, DepthKind kind, double scale)
{
  if (!e || !intensity) return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames: null");
  if (e->n_frames == 0) return fail(PHOVO_E_NOT_READY, "upload_frames: reserve_frames first");
  if (count < 0 || first_frame < 0 || first_frame + count > e->n_frames)
    return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames: frame range out of the reserved pool");
  if ((roles & PHOVO_ROLE_BOTH) == 0) return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames: roles empty");
  if ((roles & PHOVO_ROLE_SOURCE) && !depth) return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames: a source frame needs depth");
  const bool bi_target = e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE && (roles & PHOVO_ROLE_TARGET);
  if (bi_target && !depth)
    return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames: under the bi-objective a target frame needs depth");
  if (!(roles & PHOVO_ROLE_SOURCE) && !bi_target) kind = DEPTH_NONE;
  if (count == 0) return PHOVO_OK;
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(quiesce(e));                 // (an alignment in flight may be reading the frames about to be replaced)
  const int chunk_cap = count < STAGE_CHUNK ? count : STAGE_CHUNK;
  // Two staging halves: while the pyramid kernels of chunk i read one half on the engine's stream, chunk i + 1 is copied
  // into the other on the copy stream (events order each half: copied -> built -> copied again).
  const bool two_halves = count > chunk_cap;
  int st = ensure_stage(e, two_halves ? 2 * chunk_cap : chunk_cap, kind == DEPTH_F64, kind == DEPTH_U16);
  if (st != PHOVO_OK) return st;
  const size_t px = (size_t)e->width * (size_t)e->height;
  // whatever the engine's stream still does with the staging buffers (a previous upload) is over first
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  // an error half way must not leave a copy from the caller's memory in flight when this function returns
  auto drain = [&](int status) {
    (void)hipStreamSynchronize(e->copy_stream);
    (void)hipStreamSynchronize(e->stream);
    (void)quiesce(e);
    return status;
  };
  int chunk = 0;
  for (int done = 0; done < count; done += chunk_cap, chunk++) {
    const int c = count - done < chunk_cap ? count - done : chunk_cap;
    const int half = two_halves ? (chunk & 1) : 0;
    const int off = half * chunk_cap;
    if (chunk >= 2) PHOVO_DRAIN_CHECK(hipStreamWaitEvent(e->copy_stream, e->ev_built[half], 0));     // the half is free again
    st = stage_frames_h2d(e, e->d_gray + px * (size_t)off, intensity + iframe_stride * (size_t)done, istride, iframe_stride, 1, c,
                          e->copy_stream);
    if (st != PHOVO_OK) return drain(st);
    if (kind == DEPTH_F64)
      st = stage_frames_h2d(e, e->d_depth + px * (size_t)off, static_cast<const char *>(depth) + dframe_stride * (size_t)done,
                            dstride, dframe_stride, sizeof(double), c, e->copy_stream);
    else if (kind == DEPTH_U16)
      st = stage_frames_h2d(e, e->d_depth16 + px * (size_t)off, static_cast<const char *>(depth) + dframe_stride * (size_t)done,
                            dstride, dframe_stride, sizeof(uint16_t), c, e->copy_stream);
    if (st != PHOVO_OK) return drain(st);
    PHOVO_DRAIN_CHECK(hipEventRecord(e->ev_copied[half], e->copy_stream));
    PHOVO_DRAIN_CHECK(hipStreamWaitEvent(e->stream, e->ev_copied[half], 0));
    st = build_pyramids(e, first_frame + done, c, roles, kind, scale, off);
    if (st != PHOVO_OK) return drain(st);
    PHOVO_DRAIN_CHECK(hipEventRecord(e->ev_built[half], e->stream));
  }
  // the caller's buffers may be reused on return, and the staging buffers by the next upload
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->copy_stream));
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  e->ingest_pending = false;
  for (size_t i = (size_t)first_frame * PHOVO_MAX_LEVELS; i < (size_t)(first_frame + count) * PHOVO_MAX_LEVELS; i++)
    e->frame_roles[i] |= (unsigned char)(roles & PHOVO_ROLE_BOTH);
  return PHOVO_OK;
}

int phovo_engine_upload_frame(phovo_engine *e, int frame, int roles,
                              const uint8_t *intensity, size_t intensity_stride,
                              const double *depth, size_t depth_stride)
{
  return upload_batch(e, frame, 1, roles, intensity, intensity_stride, 0, depth, depth_stride, 0, DEPTH_F64, 1.0);
}

int phovo_engine_upload_frame_u16(phovo_engine *e, int frame, int roles,
                                  const uint8_t *intensity, size_t intensity_stride,
                                  const uint16_t *depth, size_t depth_stride, double depth_scale)
{
  return upload_batch(e, frame, 1, roles, intensity, intensity_stride, 0, depth, depth_stride, 0, DEPTH_U16, depth_scale);
}

int phovo_engine_upload_frames(phovo_engine *e, int first_frame, int count, int roles,
                               const uint8_t *intensity, size_t intensity_stride, size_t intensity_frame_stride,
                               const double *depth, size_t depth_stride, size_t depth_frame_stride)
{
  return upload_batch(e, first_frame, count, roles, intensity, intensity_stride, intensity_frame_stride,
                      depth, depth_stride, depth_frame_stride, DEPTH_F64, 1.0);
}

int phovo_engine_upload_frames_u16(phovo_engine *e, int first_frame, int count, int roles,
                                   const uint8_t *intensity, size_t intensity_stride, size_t intensity_frame_stride,
                                   const uint16_t *depth, size_t depth_stride, size_t depth_frame_stride,
                                   double depth_scale)
{
  return upload_batch(e, first_frame, count, roles, intensity, intensity_stride, intensity_frame_stride,
                      depth, depth_stride, depth_frame_stride, DEPTH_U16, depth_scale);
}

/* ---- frames in device memory (phovo_hip.h) ---- */

// Everything phovo_engine_upload_frames_device refuses about one descriptor, for `count` frames of w x h.
static int ingest_check_image(const phovo_engine *e, const char *which, const phovo_device_image *img, bool is_depth,
                              int count, int w, int h)
{
  const std::string who = std::string("upload_frames_device: ") + which;
  const int bpp = ingest_source_pixel_bytes(img->format);
  if (bpp == 0) return fail(PHOVO_E_INVALID_ARGUMENT, who + ".format is not a PHOVO_IMAGE_* value");
  const bool depth_format = img->format == PHOVO_IMAGE_F64 || img->format == PHOVO_IMAGE_F32 ||
                            img->format == PHOVO_IMAGE_F16 || img->format == PHOVO_IMAGE_U16;
  if (depth_format != is_depth)
    return fail(PHOVO_E_INVALID_ARGUMENT, who + (is_depth ? ".format is an intensity format" : ".format is a depth format"));
  if (img->reserved != 0) return fail(PHOVO_E_INVALID_ARGUMENT, who + ".reserved must be 0");
  if (!img->data) return fail(PHOVO_E_INVALID_ARGUMENT, who + ".data is null");
  const size_t row = (size_t)w * (size_t)bpp;
  if (img->row_stride_bytes < row) return fail(PHOVO_E_INVALID_ARGUMENT, who + ".row_stride_bytes is smaller than a row");
  const size_t frame_extent = (size_t)(h - 1) * img->row_stride_bytes + row;
  if (count > 1 && img->frame_stride_bytes < frame_extent)
    return fail(PHOVO_E_INVALID_ARGUMENT, who + ".frame_stride_bytes makes consecutive frames overlap");
  hipPointerAttribute_t attr{};
  const hipError_t he = hipPointerGetAttributes(&attr, img->data);
  if (he != hipSuccess) {
    (void)hipGetLastError();                     // (an unregistered host pointer is an error of the query, not of the device)
    return fail(PHOVO_E_INVALID_ARGUMENT, who + ".data is not device memory (" + hipGetErrorString(he) + ")");
  }
  if (attr.type != hipMemoryTypeDevice || attr.isManaged)
    return fail(PHOVO_E_INVALID_ARGUMENT, who + ".data is not plain device memory (host, pinned or managed memory)");
  if (attr.device != e->device)
    return fail(PHOVO_E_INVALID_ARGUMENT, who + ".data belongs to device " + std::to_string(attr.device) +
                                              ", the engine to device " + std::to_string(e->device));
  // the packing kernel reads [data, data + extent): it must lie inside the allocation (where the runtime knows its range)
  hipDeviceptr_t base = nullptr;
  size_t bytes = 0;
  if (hipMemGetAddressRange(&base, &bytes, const_cast<void *>(img->data)) == hipSuccess) {
    const size_t extent = (size_t)(count - 1) * (count > 1 ? img->frame_stride_bytes : 0) + frame_extent;
    const size_t offset = (size_t)(static_cast<const char *>(img->data) - static_cast<const char *>(base));
    if (offset > bytes || extent > bytes - offset)
      return fail(PHOVO_E_INVALID_ARGUMENT, who + ".data: the frames reach beyond the end of the allocation");
  } else {                                       // (no range, no bound on what the kernel would read)
    (void)hipGetLastError();
    return fail(PHOVO_E_INVALID_ARGUMENT, who + ".data: the runtime cannot name the allocation it belongs to");
  }
  return PHOVO_OK;
}

}  // extern "C"

int phovo_hip::ingest_check(const phovo_engine *e, int count, int roles, const phovo_device_image *intensity,
                            const phovo_device_image *depth, double depth_scale, int w, int h)
{
  if (!e || !intensity) return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: null engine or intensity");
  if ((roles & PHOVO_ROLE_BOTH) == 0) return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: roles empty");
  if ((roles & PHOVO_ROLE_SOURCE) && !depth)
    return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: depth is null, a source frame needs it");
  if (e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE && (roles & PHOVO_ROLE_TARGET) && !depth)
    return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: depth is null, under the bi-objective a target frame needs it");
  if (!std::isfinite(depth_scale)) return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: depth_scale is not finite");
  if (depth && depth->format == PHOVO_IMAGE_F64 && depth_scale != 1.0)
    return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: depth_scale must be 1 with PHOVO_IMAGE_F64");
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  int st = ingest_check_image(e, "intensity", intensity, false, count, w, h);
  if (st == PHOVO_OK && depth) st = ingest_check_image(e, "depth", depth, true, count, w, h);
  return st;
}

extern "C" {

int phovo_engine_upload_frames_device(phovo_engine *e, int first_frame, int count, int roles,
                                      const phovo_device_image *intensity, const phovo_device_image *depth,
                                      double depth_scale, void *stream)
{
  if (!e || !intensity) return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: null engine or intensity");
  if (e->n_frames == 0) return fail(PHOVO_E_NOT_READY, "upload_frames_device: reserve_frames first");
  if (count < 0 || first_frame < 0 || first_frame + count > e->n_frames)
    return fail(PHOVO_E_INVALID_ARGUMENT, "upload_frames_device: first_frame / count out of the reserved pool");
  int st = ingest_check(e, count, roles, intensity, depth, depth_scale, e->width, e->height);
  if (st != PHOVO_OK) return st;
  const bool bi_target = e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE && (roles & PHOVO_ROLE_TARGET);
  const bool want_depth = (roles & PHOVO_ROLE_SOURCE) || bi_target;
  // u16 goes to the u16 staging and is scaled by the producers, as in a host u16 upload; everything else is staged as
  // fp64 metres (f32 / f16 scaled by the packing kernel)
  const DepthKind kind = !want_depth ? DEPTH_NONE : depth->format == PHOVO_IMAGE_U16 ? DEPTH_U16 : DEPTH_F64;
  if (count == 0) return PHOVO_OK;
  hipStream_t producer = static_cast<hipStream_t>(stream);
  PHOVO_HIP_CHECK(quiesce(e));                 // (an alignment in flight may be reading the frames about to be replaced)
  const int chunk_cap = count < STAGE_CHUNK ? count : STAGE_CHUNK;
  const bool two_halves = count > chunk_cap;   // the host path's two staging halves, here both on the engine's stream
  st = ensure_stage(e, two_halves ? 2 * chunk_cap : chunk_cap, kind == DEPTH_F64, kind == DEPTH_U16);
  if (st != PHOVO_OK) return st;
  const size_t px = (size_t)e->width * (size_t)e->height;
  // nothing of the caller's may be read after an error return
  auto drain = [&](int status) { (void)hipStreamSynchronize(e->stream); return status; };
  // the producer's work so far comes first
  PHOVO_DRAIN_CHECK(hipEventRecord(e->ev_ingest_produced, producer));
  PHOVO_DRAIN_CHECK(hipStreamWaitEvent(e->stream, e->ev_ingest_produced, 0));
  phovo_ingest_record rec{};
  for (int done = 0; done < count; done += chunk_cap, rec.chunks++) {
    const int c = count - done < chunk_cap ? count - done : chunk_cap;
    const int off = two_halves ? (rec.chunks & 1) * chunk_cap : 0;
    bool wide = false;
    PHOVO_DRAIN_CHECK(ingest_pack(intensity->format,
                                   static_cast<const char *>(intensity->data) + intensity->frame_stride_bytes * (size_t)done,
                                   intensity->row_stride_bytes, intensity->frame_stride_bytes, c, e->width, e->height, 1.0,
                                   e->d_gray + px * (size_t)off, &wide, e->stream));
    (wide ? rec.wide_launches : rec.scalar_launches)++;
    if (kind != DEPTH_NONE) {
      void *dst = kind == DEPTH_U16 ? static_cast<void *>(e->d_depth16 + px * (size_t)off)
                                    : static_cast<void *>(e->d_depth + px * (size_t)off);
      PHOVO_DRAIN_CHECK(ingest_pack(depth->format,
                                     static_cast<const char *>(depth->data) + depth->frame_stride_bytes * (size_t)done,
                                     depth->row_stride_bytes, depth->frame_stride_bytes, c, e->width, e->height, depth_scale,
                                     dst, &wide, e->stream));
      (wide ? rec.wide_launches : rec.scalar_launches)++;
    }
    if (done + c == count) {                   // the caller's memory has been read: its stream may go on behind this point
      PHOVO_DRAIN_CHECK(hipEventRecord(e->ev_ingest_read, e->stream));
      PHOVO_DRAIN_CHECK(hipStreamWaitEvent(producer, e->ev_ingest_read, 0));
    }
    st = build_pyramids(e, first_frame + done, c, roles, kind, kind == DEPTH_U16 ? depth_scale : 1.0, off);
    if (st != PHOVO_OK) return drain(st);
  }
  PHOVO_DRAIN_CHECK(hipEventRecord(e->ev_ingested, e->stream));
  e->ingest_pending = true;
  e->last_ingest = rec;
  for (size_t i = (size_t)first_frame * PHOVO_MAX_LEVELS; i < (size_t)(first_frame + count) * PHOVO_MAX_LEVELS; i++)
    e->frame_roles[i] |= (unsigned char)(roles & PHOVO_ROLE_BOTH);
  return PHOVO_OK;
}

int phovo_engine_last_ingest(const phovo_engine *e, phovo_ingest_record *out)
{
  if (!e || !out) return fail(PHOVO_E_INVALID_ARGUMENT, "last_ingest: null");
  *out = e->last_ingest;
  return PHOVO_OK;
}

static int plane_access_check(const phovo_engine *e, int frame, int level)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "level planes: null engine");
  if (e->n_frames == 0) return fail(PHOVO_E_NOT_READY, "level planes: reserve_frames first");
  if (frame < 0 || frame >= e->n_frames) return fail(PHOVO_E_INVALID_ARGUMENT, "level planes: frame index out of range");
  if (level < 0 || level >= e->cfg.num_levels) return fail(PHOVO_E_INVALID_ARGUMENT, "level planes: level out of range");
  if (!e->levels[level].stored) return fail(PHOVO_E_NOT_READY, "level planes: level is not resident (max_num_iterations == 0 and build_all_levels off)");
  return PHOVO_OK;
}

int phovo_engine_set_level_planes(phovo_engine *e, int frame, int level,
                                  const double *intensity, const double *depth,
                                  const double *grad_x, const double *grad_y)
{
  const int st = plane_access_check(e, frame, level);
  if (st != PHOVO_OK) return st;
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(quiesce(e));
  const LevelPool &lv = e->levels[level];
  unsigned char *base = lv.planes + (size_t)frame * lv.frame_bytes;
  const double *srcs[4] = {intensity, depth, grad_x, grad_y};
  for (int p = 0; p < 4; p++) {
    if (!srcs[p]) continue;
    if (e->ext.plane_storage == PHOVO_STORAGE_F64) {
      PHOVO_HIP_CHECK(hipMemcpyAsync(base + lv.plane_off[p], srcs[p], sizeof(double) * (size_t)lv.n,
                                     hipMemcpyHostToDevice, e->stream));
    } else {                                   // round to the storage type on the device, like the producers do
      PHOVO_HIP_CHECK(hipMemcpyAsync(e->d_scratch, srcs[p], sizeof(double) * (size_t)lv.n, hipMemcpyHostToDevice, e->stream));
      PHOVO_HIP_CHECK(pyr_store_plane(e->d_scratch, 0, 1, lv.n, base + lv.plane_off[p], lv.frame_bytes,
                                      e->ext.plane_storage, p == PLANE_D, e->stream));
      PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
  }
  if (lv.rec_off && (intensity || grad_x || grad_y))                    // bilinear sampling: this frame's tap records follow its planes
    PHOVO_HIP_CHECK(pyr_build_tap_records(lv.planes + (size_t)frame * lv.frame_bytes, lv.frame_bytes, lv.plane_off, lv.rec_off,
                                          1, lv.n, e->ext.plane_storage, e->stream));
  if (lv.gain_off) {               // bi-objective: the gain always, the depth gradients when the depth changed (max depth in force)
    const double *fb = reinterpret_cast<const double *>(base);
    const size_t fstride = lv.frame_bytes / sizeof(double);
    if (depth) {
      const int bst = build_biobjective_target(e, level, frame, 1);
      if (bst != PHOVO_OK) return bst;
    } else {
      PHOVO_HIP_CHECK(pyr_depth_gain(fb, fstride, lv.plane_off[PLANE_I] / sizeof(double), lv.plane_off[PLANE_D] / sizeof(double),
                                     lv.gain_off / sizeof(double), 1, lv.n, e->stream));
    }
  }
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  unsigned char &roles = e->frame_roles[(size_t)frame * PHOVO_MAX_LEVELS + (size_t)level];     // (this level only)
  if (depth) roles |= PHOVO_ROLE_SOURCE;
  if (grad_x || grad_y) roles |= PHOVO_ROLE_TARGET;
  return PHOVO_OK;
}

int phovo_engine_get_level_depth_gradients(const phovo_engine *e, int frame, int level, double *grad_x, double *grad_y)
{
  const int st = plane_access_check(e, frame, level);
  if (st != PHOVO_OK) return st;
  const LevelPool &lv = e->levels[level];
  if (!lv.gain_off) return fail(PHOVO_E_UNSUPPORTED, "level depth gradients: the objective is not PHOVO_OBJECTIVE_BIOBJECTIVE");
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  const unsigned char *base = lv.planes + (size_t)frame * lv.frame_bytes;
  if (grad_x) PHOVO_HIP_CHECK(hipMemcpy(grad_x, base + lv.dgx_off, sizeof(double) * (size_t)lv.n, hipMemcpyDeviceToHost));
  if (grad_y) PHOVO_HIP_CHECK(hipMemcpy(grad_y, base + lv.dgy_off, sizeof(double) * (size_t)lv.n, hipMemcpyDeviceToHost));
  return PHOVO_OK;
}

int phovo_engine_get_level_depth_gain(const phovo_engine *e, int frame, int level, double *gain)
{
  const int st = plane_access_check(e, frame, level);
  if (st != PHOVO_OK) return st;
  if (!gain) return fail(PHOVO_E_INVALID_ARGUMENT, "level depth gain: null");
  const LevelPool &lv = e->levels[level];
  if (!lv.gain_off) return fail(PHOVO_E_UNSUPPORTED, "level depth gain: the objective is not PHOVO_OBJECTIVE_BIOBJECTIVE");
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  PHOVO_HIP_CHECK(hipMemcpy(gain, lv.planes + (size_t)frame * lv.frame_bytes + lv.gain_off, sizeof(double), hipMemcpyDeviceToHost));
  return PHOVO_OK;
}

int phovo_engine_get_level_planes(const phovo_engine *e, int frame, int level,
                                  double *intensity, double *depth, double *grad_x, double *grad_y)
{
  const int st = plane_access_check(e, frame, level);
  if (st != PHOVO_OK) return st;
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  const LevelPool &lv = e->levels[level];
  const unsigned char *base = lv.planes + (size_t)frame * lv.frame_bytes;
  double *dsts[4] = {intensity, depth, grad_x, grad_y};
  PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
  for (int p = 0; p < 4; p++) {
    if (!dsts[p]) continue;
    if (e->ext.plane_storage == PHOVO_STORAGE_F64) {
      PHOVO_HIP_CHECK(hipMemcpy(dsts[p], base + lv.plane_off[p], sizeof(double) * (size_t)lv.n, hipMemcpyDeviceToHost));
    } else {
      PHOVO_HIP_CHECK(pyr_load_plane(base + lv.plane_off[p], lv.n, e->d_scratch, e->ext.plane_storage, p == PLANE_D, e->stream));
      PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));
      PHOVO_HIP_CHECK(hipMemcpy(dsts[p], e->d_scratch, sizeof(double) * (size_t)lv.n, hipMemcpyDeviceToHost));
    }
  }
  return PHOVO_OK;
}


}  // extern "C"
