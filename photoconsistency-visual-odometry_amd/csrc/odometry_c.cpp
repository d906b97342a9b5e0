// The single-pair class surface of the C ABI (phovo_odometry_*), which mirrors
// phovo::Analytic::CPhotoconsistencyOdometryAnalytic (CPhotoconsistencyOdometryAnalytic.h:428-607): a client of the engine,
// with one engine of two frames of its own.

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "engine_internal.hpp"

using namespace phovo_hip;

struct phovo_odometry {
  phovo_engine *engine = nullptr;
  bool have_source = false, have_target = false, optimized = false;
  double init_state[6] = {0, 0, 0, 0, 0, 0};
  double state[6] = {0, 0, 0, 0, 0, 0};          // m_StateVector.setZero()  :432
  phovo_pair_report report{};
  phovo_trust_region_report tr_report{};         // trust-region objective: the solver record of the last Optimize()
  bool have_tr_report = false;
  double illumination[2] = {0, 0};               // affine-illumination objective: (alpha, beta) of the last Optimize()
  bool have_illumination = false;
  phovo_geometric_report geo_report{};           // photometric-geometric objective: the record of the last Optimize()
  bool have_geo_report = false;
  phovo_robust_report rob_report{};              // robust inverse-compositional objective: the record of the last Optimize()
  bool have_rob_report = false;
  phovo_semidense_report sd_report{};            // semi-dense inverse-compositional objective: the record of the last Optimize()
  bool have_sd_report = false;
  bool have_prior = false;                       // phovo_odometry_set_pose_prior: every Optimize() carries it until it is cleared
  double prior_state[6] = {0, 0, 0, 0, 0, 0};
  double prior_information[36] = {};
  phovo_prior_report prior_report{};             // the record of the last Optimize(), if it carried a prior
  bool have_prior_report = false;
};

namespace {

// The inverse-compositional objectives read the source's gradient planes, which are a target upload's.
int source_role(const phovo_odometry *o)
{
  const bool inverse = o && (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL ||
                             o->engine->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST ||
                             o->engine->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE);
  return inverse ? PHOVO_ROLE_BOTH : PHOVO_ROLE_SOURCE;
}

int odometry_set_frame(phovo_odometry *o, int slot, int role, const uint8_t *intensity, size_t istride,
                       const double *depth, size_t dstride, int width, int height)
{
  if (!o || !intensity) return fail(PHOVO_E_INVALID_ARGUMENT, "Set*Frame: null");
  if (width < 1 || height < 1) return fail(PHOVO_E_INVALID_ARGUMENT, "Set*Frame: empty image");
  phovo_engine *e = o->engine;
  if (e->n_frames == 0 || e->width != width || e->height != height) {
    const int st = phovo_engine_reserve_frames(e, 2, width, height);
    if (st != PHOVO_OK) return st;
    o->have_source = o->have_target = false;
  }
  const int st = phovo_engine_upload_frame(e, slot, role, intensity, istride, depth, dstride);
  if (st != PHOVO_OK) return st;
  if (slot == 0) o->have_source = true; else o->have_target = true;
  o->optimized = false;
  return PHOVO_OK;
}

int odometry_set_frame_device(phovo_odometry *o, int slot, int role, const phovo_device_image *intensity,
                              const phovo_device_image *depth, double depth_scale, int width, int height, void *stream)
{
  if (!o || !intensity) return fail(PHOVO_E_INVALID_ARGUMENT, "Set*FrameDevice: null odometry or intensity");
  if (width < 1 || height < 1) return fail(PHOVO_E_INVALID_ARGUMENT, "Set*FrameDevice: empty image");
  phovo_engine *e = o->engine;
  if (e->n_frames == 0 || e->width != width || e->height != height) {
    // (every refusal comes before the pool is dropped for the new size)
    int st = ingest_check(e, 1, role, intensity, depth, depth_scale, width, height);
    if (st != PHOVO_OK) return st;
    st = phovo_engine_reserve_frames(e, 2, width, height);
    if (st != PHOVO_OK) return st;
    o->have_source = o->have_target = false;
  }
  const int st = phovo_engine_upload_frames_device(e, slot, 1, role, intensity, depth, depth_scale, stream);
  if (st != PHOVO_OK) return st;
  if (slot == 0) o->have_source = true; else o->have_target = true;
  o->optimized = false;
  return PHOVO_OK;
}

}  // namespace

extern "C" {

int phovo_odometry_create(int device, phovo_odometry **out)
{
  if (!out) return fail(PHOVO_E_INVALID_ARGUMENT, "phovo_odometry_create: null");
  *out = nullptr;
  phovo_engine *e = nullptr;
  const int st = phovo_engine_create(device, &e);
  if (st != PHOVO_OK) return st;
  phovo_odometry *o = new (std::nothrow) phovo_odometry();
  if (!o) { phovo_engine_destroy(e); return fail(PHOVO_E_INVALID_ARGUMENT, "out of host memory"); }
  o->engine = e;
  *out = o;
  return PHOVO_OK;
}

int phovo_odometry_destroy(phovo_odometry *o)
{
  if (!o) return PHOVO_OK;
  phovo_engine_destroy(o->engine);
  delete o;
  return PHOVO_OK;
}

int phovo_odometry_set_config(phovo_odometry *o, const phovo_config *cfg)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_config: null");
  const int st = phovo_engine_set_config(o->engine, cfg);
  if (st == PHOVO_OK) o->have_source = o->have_target = o->optimized = false;
  return st;
}

int phovo_odometry_set_extensions(phovo_odometry *o, const phovo_extensions *ext)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_extensions: null");
  const int before = o->engine->ext.plane_storage;
  const int st = phovo_engine_set_extensions(o->engine, ext);
  if (st == PHOVO_OK && ext->plane_storage != before) o->have_source = o->have_target = o->optimized = false;
  return st;
}

int phovo_odometry_set_objective(phovo_odometry *o, int objective)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_objective: null");
  const int before = o->engine->objective;
  const int st = phovo_engine_set_objective(o->engine, objective);
  if (st == PHOVO_OK && objective != before) o->have_source = o->have_target = o->optimized = false;
  return st;
}

int phovo_odometry_set_trust_region_options(phovo_odometry *o, const phovo_trust_region_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_trust_region_options: null");
  return phovo_engine_set_trust_region_options(o->engine, opt);
}

int phovo_odometry_get_trust_region_options(const phovo_odometry *o, phovo_trust_region_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "get_trust_region_options: null");
  return phovo_engine_get_trust_region_options(o->engine, opt);
}

int phovo_odometry_set_geometric_options(phovo_odometry *o, const phovo_geometric_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_geometric_options: null");
  return phovo_engine_set_geometric_options(o->engine, opt);
}

int phovo_odometry_get_geometric_options(const phovo_odometry *o, phovo_geometric_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "get_geometric_options: null");
  return phovo_engine_get_geometric_options(o->engine, opt);
}

int phovo_odometry_set_robust_options(phovo_odometry *o, const phovo_robust_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_robust_options: null");
  return phovo_engine_set_robust_options(o->engine, opt);
}

int phovo_odometry_get_robust_options(const phovo_odometry *o, phovo_robust_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "get_robust_options: null");
  return phovo_engine_get_robust_options(o->engine, opt);
}

int phovo_odometry_set_semidense_options(phovo_odometry *o, const phovo_semidense_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_semidense_options: null");
  return phovo_engine_set_semidense_options(o->engine, opt);
}

int phovo_odometry_get_semidense_options(const phovo_odometry *o, phovo_semidense_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "get_semidense_options: null");
  return phovo_engine_get_semidense_options(o->engine, opt);
}

int phovo_odometry_set_latency_forms(phovo_odometry *o, int on)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_latency_forms: null");
  return phovo_engine_set_latency_forms(o->engine, on);
}

int phovo_odometry_read_configuration_file(phovo_odometry *o, const char *path)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "ReadConfigurationFile: null");
  phovo_config c;
  if (o->engine->objective == PHOVO_OBJECTIVE_TRUST_REGION) {    // CPhotoconsistencyOdometryCeres::ReadConfigurationFile
    phovo_trust_region_options opt;
    int st = read_trust_region_file(path, &c, &opt);
    if (st != PHOVO_OK) return st;
    st = phovo_engine_set_trust_region_options(o->engine, &opt);
    if (st != PHOVO_OK) return st;
    return phovo_odometry_set_config(o, &c);
  }
  int st = read_config_file(path, &c);
  if (st != PHOVO_OK) return st;
  if (o->engine->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) {      // its two optional keys; absent: the defaults
    phovo_geometric_options g;
    st = read_geometric_file(path, &g);
    if (st != PHOVO_OK) return st;
    st = phovo_engine_set_geometric_options(o->engine, &g);
    if (st != PHOVO_OK) return st;
  }
  if (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {          // its optional key; absent: the defaults
    phovo_semidense_options sd;
    st = read_semidense_file(path, &sd);
    if (st != PHOVO_OK) return st;
    st = phovo_engine_set_semidense_options(o->engine, &sd);
    if (st != PHOVO_OK) return st;
  }
  phovo_extensions x;                        // optional keys; a reference yml has none -> everything stays off
  st = read_extensions_file(path, &x);
  if (st != PHOVO_OK) return st;
  st = phovo_odometry_set_extensions(o, &x);
  if (st != PHOVO_OK) return st;
  return phovo_odometry_set_config(o, &c);
}

int phovo_odometry_set_min_depth(phovo_odometry *o, double v)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "SetMinDepth: null");
  o->engine->min_depth = v;
  return PHOVO_OK;
}

int phovo_odometry_set_max_depth(phovo_odometry *o, double v)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "SetMaxDepth: null");
  o->engine->max_depth = v;
  return PHOVO_OK;
}

int phovo_odometry_set_intrinsic_matrix(phovo_odometry *o, const double k[9])
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "SetIntrinsicMatrix: null");
  return phovo_engine_set_intrinsic_matrix(o->engine, k);
}

int phovo_odometry_set_source_frame(phovo_odometry *o, const uint8_t *intensity, size_t istride,
                                    const double *depth, size_t dstride, int width, int height)
{
  if (!depth) return fail(PHOVO_E_INVALID_ARGUMENT, "SetSourceFrame: depth is required");
  return odometry_set_frame(o, 0, source_role(o), intensity, istride, depth, dstride, width, height);
}

int phovo_odometry_set_target_frame(phovo_odometry *o, const uint8_t *intensity, size_t istride,
                                    const double *depth, size_t dstride, int width, int height)
{
  if (o && o->engine->objective == PHOVO_OBJECTIVE_BIOBJECTIVE) {       // the target keeps its depth  (...BiObjective.h:573)
    if (!depth) return fail(PHOVO_E_INVALID_ARGUMENT, "SetTargetFrame: the bi-objective needs the target's depth");
    return odometry_set_frame(o, 1, PHOVO_ROLE_TARGET, intensity, istride, depth, dstride, width, height);
  }
  if (o && o->engine->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) {      // the target's depth plane is a source upload's
    if (!depth) return fail(PHOVO_E_INVALID_ARGUMENT, "SetTargetFrame: the photometric-geometric objective needs the target's depth");
    return odometry_set_frame(o, 1, PHOVO_ROLE_BOTH, intensity, istride, depth, dstride, width, height);
  }
  (void)depth; (void)dstride;                      // "Depth image is ignored"  :478
  return odometry_set_frame(o, 1, PHOVO_ROLE_TARGET, intensity, istride, nullptr, 0, width, height);
}

int phovo_odometry_set_source_frame_device(phovo_odometry *o, const phovo_device_image *intensity,
                                           const phovo_device_image *depth, double depth_scale, int width, int height,
                                           void *stream)
{
  if (!depth) return fail(PHOVO_E_INVALID_ARGUMENT, "SetSourceFrameDevice: depth is required");
  return odometry_set_frame_device(o, 0, source_role(o), intensity, depth, depth_scale, width, height, stream);
}

int phovo_odometry_set_target_frame_device(phovo_odometry *o, const phovo_device_image *intensity,
                                           const phovo_device_image *depth, double depth_scale, int width, int height,
                                           void *stream)
{
  if (o && o->engine->objective == PHOVO_OBJECTIVE_BIOBJECTIVE) {       // the target keeps its depth
    if (!depth) return fail(PHOVO_E_INVALID_ARGUMENT, "SetTargetFrameDevice: the bi-objective needs the target's depth");
    return odometry_set_frame_device(o, 1, PHOVO_ROLE_TARGET, intensity, depth, depth_scale, width, height, stream);
  }
  if (o && o->engine->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) {
    if (!depth) return fail(PHOVO_E_INVALID_ARGUMENT, "SetTargetFrameDevice: the photometric-geometric objective needs the target's depth");
    return odometry_set_frame_device(o, 1, PHOVO_ROLE_BOTH, intensity, depth, depth_scale, width, height, stream);
  }
  // "Depth image is ignored"  :478
  return odometry_set_frame_device(o, 1, PHOVO_ROLE_TARGET, intensity, nullptr, 1.0, width, height, stream);
}

int phovo_odometry_set_initial_state_vector(phovo_odometry *o, const double state[6])
{
  if (!o || !state) return fail(PHOVO_E_INVALID_ARGUMENT, "SetInitialStateVector: null");
  std::memcpy(o->init_state, state, sizeof(o->init_state));
  std::memcpy(o->state, state, sizeof(o->state));   // m_StateVector = initialStateVector  :496
  return PHOVO_OK;
}

// visualizeIterations, headless (...Analytic.h:515-517,359-362,551-557).  The reference fills a warped source image
// while it computes the residuals -- warped(tr, tc) = I0(r, c) for every source pixel that passes the depth gate and lands
// in bounds, last raster writer wins, zero elsewhere -- and after every iteration that does NOT end the level shows
// |I1 - warped| in a window and waits for a key.  Here, when the configuration asks for it AND PHOVO_VISUALIZE_DIR names a
// directory, Optimize() runs one iteration per launch (same kernels, same arithmetic as the fused loop: the state a launch
// ends with is the state the next one starts from) and writes that image as
//   <dir>/optimize_imgDiff_level<L>_iteration<N>.pgm   (8 bit: |diff| * 255, rounded; what imshow does to a [0, 1] image)
// Display code, on the host and outside every timed region; without the directory the key is parsed and ignored as before.
static int write_iteration_image(phovo_engine *e, int level, int iteration, const double pre_state[6], const char *dir)
{
  const LevelPool &lv = e->levels[level];
  std::vector<double> i0((size_t)lv.n), d0((size_t)lv.n), i1((size_t)lv.n), warped((size_t)lv.n, 0.0);
  int st = phovo_engine_get_level_planes(e, 0, level, i0.data(), d0.data(), nullptr, nullptr);
  if (st != PHOVO_OK) return st;
  st = phovo_engine_get_level_planes(e, 1, level, i1.data(), nullptr, nullptr, nullptr);
  if (st != PHOVO_OK) return st;
  double rt[16];
  phovo_eigen_pose(pre_state, rt);
  const double sc = 1.0 / std::pow(2, level);
  const double fx = e->K[0] * sc, fy = e->K[4] * sc, ox = e->K[2] * sc, oy = e->K[5] * sc;
  const double ifx = 1.f / fx, ify = 1.f / fy;
  for (int r = 0; r < lv.h; r++)
    for (int c = 0; c < lv.w; c++) {
      const double pz = d0[(size_t)r * lv.w + c];
      if (!(e->min_depth < pz && pz < e->max_depth)) continue;                     // :280
      const double px = (c - ox) * pz * ifx, py = (r - oy) * pz * ify;            // :282-283
      const double X = ((rt[0] * px + rt[1] * py) + rt[2] * pz) + rt[3];           // :291
      const double Y = ((rt[4] * px + rt[5] * py) + rt[6] * pz) + rt[7];
      const double Z = ((rt[8] * px + rt[9] * py) + rt[10] * pz) + rt[11];
      const double iz = 1.0 / Z;
      const double rr = std::round((Y * fy) * iz + oy), rc = std::round((X * fx) * iz + ox);   // :294-298
      if (rr >= 0 && rr < (double)lv.h && rc >= 0 && rc < (double)lv.w)            // :302-303
        warped[(size_t)rr * lv.w + (size_t)rc] = i0[(size_t)r * lv.w + c];         // :361
    }
  std::vector<unsigned char> img((size_t)lv.n);
  for (int k = 0; k < lv.n; k++) {
    const double v = std::fabs(i1[(size_t)k] - warped[(size_t)k]) * 255.0;         // cv::absdiff  :554
    img[(size_t)k] = (unsigned char)(v >= 255.0 ? 255 : (int)std::lrint(v));
  }
  const std::string path = std::string(dir) + "/optimize_imgDiff_level" + std::to_string(level) + "_iteration" +
                           std::to_string(iteration) + ".pgm";
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return fail(PHOVO_E_IO, "visualizeIterations: cannot write " + path);
  std::fprintf(f, "P5\n%d %d\n255\n", lv.w, lv.h);
  const bool ok = std::fwrite(img.data(), 1, img.size(), f) == img.size();
  std::fclose(f);
  return ok ? PHOVO_OK : fail(PHOVO_E_IO, "visualizeIterations: short write to " + path);
}

static int optimize_visualized(phovo_odometry *o, const char *dir)
{
  phovo_engine *e = o->engine;
  const phovo_config full = e->cfg;
  const int src = 0, tgt = 1;
  phovo_pair_report total{};
  int st = PHOVO_OK;
  for (int l = full.num_levels - 1; l >= 0 && st == PHOVO_OK; l--) {               // coarse to fine  :502-503
    total.iterations[l] = 1;                                                       // a level without iterations still runs the loop once
    if (full.max_num_iterations[l] <= 0) continue;
    phovo_config one = full;
    for (int m = 0; m < one.num_levels; m++) one.max_num_iterations[m] = m == l ? 1 : 0;
    one.visualize_iterations = 0;
    for (int it = 1;; it++) {
      double pre[6];
      std::memcpy(pre, o->state, sizeof(pre));
      // (levels that stay resident keep the pool: only max_num_iterations changes)
      e->cfg = one;
      phovo_pair_report rep{};
      st = phovo_engine_align_pairs(e, 1, &src, &tgt, o->state, o->state, &rep);
      e->cfg = full;
      if (st != PHOVO_OK) break;
      total.iterations[l] = it;
      total.gradient_norm = rep.gradient_norm;
      total.flags |= rep.flags;
      total.valid_pixels[l] = rep.valid_pixels[l];
      const bool stop = it >= full.max_num_iterations[l] || rep.gradient_norm < full.min_gradient_norm[l] ||
                        (rep.flags & PHOVO_PAIR_NONFINITE);                       // :383,388
      if (stop) break;
      st = write_iteration_image(e, l, it, pre, dir);                              // :551-557: only when the level goes on
      if (st != PHOVO_OK) break;
    }
  }
  e->cfg = full;
  if (st != PHOVO_OK) return st;
  o->report = total;
  o->have_illumination = false;
  o->have_geo_report = false;
  o->have_rob_report = false;
  o->have_sd_report = false;
  o->optimized = true;
  return PHOVO_OK;
}

int phovo_odometry_optimize(phovo_odometry *o)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "Optimize: null");
  if (!o->have_source || !o->have_target)
    return fail(PHOVO_E_NOT_READY, "Optimize: SetSourceFrame and SetTargetFrame must be called first");
  if (o->have_prior && o->engine->objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL &&
      o->engine->objective != PHOVO_OBJECTIVE_INVERSE_ROBUST)
    return fail(PHOVO_E_UNSUPPORTED, "Optimize: a pose prior is set, which only the two inverse-compositional objectives take "
                                     "(phovo_odometry_clear_pose_prior)");
  // (the affine-illumination objective carries alpha and beta inside an enqueue only: no one-iteration-per-launch form)
  // (the photometric-geometric objective's per-level record belongs to one enqueue: likewise)
  // (the inverse-compositional objectives carry (R, t) inside a level's launch only: likewise)
  if (o->engine->cfg.visualize_iterations && o->engine->objective != PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE &&
      o->engine->objective != PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC &&
      o->engine->objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL &&
      o->engine->objective != PHOVO_OBJECTIVE_INVERSE_ROBUST &&
      o->engine->objective != PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {
    const char *dir = std::getenv("PHOVO_VISUALIZE_DIR");
    if (dir && *dir) return optimize_visualized(o, dir);
  }
  const int src = 0, tgt = 1;
  // Like the reference, Optimize() starts from the CURRENT state vector (:539 updates m_StateVector in place).
  int st;
  if (o->have_prior) {
    st = phovo_engine_enqueue_align_prior(o->engine, 1, &src, &tgt, o->state, o->prior_state, o->prior_information);
    if (st == PHOVO_OK) st = phovo_engine_fetch_results(o->engine, 1, o->state, &o->report);
  } else {
    st = phovo_engine_align_pairs(o->engine, 1, &src, &tgt, o->state, o->state, &o->report);
  }
  if (st != PHOVO_OK) return st;
  o->have_prior_report = o->have_prior;
  if (o->have_prior_report) {
    st = phovo_engine_fetch_prior_reports(o->engine, 1, &o->prior_report);
    if (st != PHOVO_OK) return st;
  }
  o->have_tr_report = o->engine->objective == PHOVO_OBJECTIVE_TRUST_REGION;
  if (o->have_tr_report) {
    st = phovo_engine_fetch_trust_region_reports(o->engine, 1, &o->tr_report);
    if (st != PHOVO_OK) return st;
  }
  o->have_illumination = o->engine->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE;
  if (o->have_illumination) {
    st = phovo_engine_fetch_illumination(o->engine, 1, o->illumination);
    if (st != PHOVO_OK) return st;
  }
  o->have_geo_report = o->engine->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC;
  if (o->have_geo_report) {
    st = phovo_engine_fetch_geometric_reports(o->engine, 1, &o->geo_report);
    if (st != PHOVO_OK) return st;
  }
  o->have_rob_report = o->engine->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST;
  if (o->have_rob_report) {
    st = phovo_engine_fetch_robust_reports(o->engine, 1, &o->rob_report);
    if (st != PHOVO_OK) return st;
  }
  o->have_sd_report = o->engine->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE;
  if (o->have_sd_report) {
    st = phovo_engine_fetch_semidense_reports(o->engine, 1, &o->sd_report);
    if (st != PHOVO_OK) return st;
  }
  o->optimized = true;
  return PHOVO_OK;
}

int phovo_odometry_get_semidense_report(const phovo_odometry *o, phovo_semidense_report *report)
{
  if (!o || !report) return fail(PHOVO_E_INVALID_ARGUMENT, "get_semidense_report: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_semidense_report: Optimize has not run");
  if (!o->have_sd_report) return fail(PHOVO_E_UNSUPPORTED, "get_semidense_report: the last Optimize ran under another objective");
  *report = o->sd_report;
  return PHOVO_OK;
}

int phovo_odometry_get_robust_report(const phovo_odometry *o, phovo_robust_report *report)
{
  if (!o || !report) return fail(PHOVO_E_INVALID_ARGUMENT, "get_robust_report: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_robust_report: Optimize has not run");
  if (!o->have_rob_report) return fail(PHOVO_E_UNSUPPORTED, "get_robust_report: the last Optimize ran under another objective");
  *report = o->rob_report;
  return PHOVO_OK;
}

int phovo_odometry_set_pose_prior(phovo_odometry *o, const double state[6], const double information[36])
{
  if (!o || !state || !information) return fail(PHOVO_E_INVALID_ARGUMENT, "set_pose_prior: null");
  for (int i = 0; i < 6; i++)
    if (!std::isfinite(state[i])) return fail(PHOVO_E_INVALID_ARGUMENT, "set_pose_prior: the prior state is not finite");
  for (int i = 0; i < 36; i++)
    if (!std::isfinite(information[i])) return fail(PHOVO_E_INVALID_ARGUMENT, "set_pose_prior: an information entry is not finite");
  for (int d = 0; d < 6; d++)
    if (information[7 * d] < 0.0) return fail(PHOVO_E_INVALID_ARGUMENT, "set_pose_prior: a negative diagonal entry");
  std::memcpy(o->prior_state, state, sizeof(o->prior_state));
  std::memcpy(o->prior_information, information, sizeof(o->prior_information));
  o->have_prior = true;
  return PHOVO_OK;
}

int phovo_odometry_clear_pose_prior(phovo_odometry *o)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "clear_pose_prior: null");
  o->have_prior = false;
  return PHOVO_OK;
}

int phovo_odometry_set_prior_options(phovo_odometry *o, const phovo_prior_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "set_prior_options: null");
  return phovo_engine_set_prior_options(o->engine, opt);
}

int phovo_odometry_get_prior_options(const phovo_odometry *o, phovo_prior_options *opt)
{
  if (!o) return fail(PHOVO_E_INVALID_ARGUMENT, "get_prior_options: null");
  return phovo_engine_get_prior_options(o->engine, opt);
}

int phovo_odometry_get_prior_report(const phovo_odometry *o, phovo_prior_report *report)
{
  if (!o || !report) return fail(PHOVO_E_INVALID_ARGUMENT, "get_prior_report: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_prior_report: Optimize has not run");
  if (!o->have_prior_report) return fail(PHOVO_E_UNSUPPORTED, "get_prior_report: the last Optimize ran without a pose prior");
  *report = o->prior_report;
  return PHOVO_OK;
}

int phovo_odometry_get_geometric_report(const phovo_odometry *o, phovo_geometric_report *report)
{
  if (!o || !report) return fail(PHOVO_E_INVALID_ARGUMENT, "get_geometric_report: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_geometric_report: Optimize has not run");
  if (!o->have_geo_report) return fail(PHOVO_E_UNSUPPORTED, "get_geometric_report: the last Optimize ran under another objective");
  *report = o->geo_report;
  return PHOVO_OK;
}

int phovo_odometry_get_illumination(const phovo_odometry *o, double alpha_beta[2])
{
  if (!o || !alpha_beta) return fail(PHOVO_E_INVALID_ARGUMENT, "get_illumination: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_illumination: Optimize has not run");
  if (!o->have_illumination) return fail(PHOVO_E_UNSUPPORTED, "get_illumination: the last Optimize ran under another objective");
  alpha_beta[0] = o->illumination[0]; alpha_beta[1] = o->illumination[1];
  return PHOVO_OK;
}

int phovo_odometry_get_optimal_state_vector(const phovo_odometry *o, double state[6])
{
  if (!o || !state) return fail(PHOVO_E_INVALID_ARGUMENT, "GetOptimalStateVector: null");
  std::memcpy(state, o->state, sizeof(o->state));
  return PHOVO_OK;
}

int phovo_odometry_get_optimal_rigid_transformation_matrix(const phovo_odometry *o, double rt[16])
{
  if (!o || !rt) return fail(PHOVO_E_INVALID_ARGUMENT, "GetOptimalRigidTransformationMatrix: null");
  return phovo_eigen_pose(o->state, rt);            // :572-578
}

int phovo_odometry_get_report(const phovo_odometry *o, phovo_pair_report *report)
{
  if (!o || !report) return fail(PHOVO_E_INVALID_ARGUMENT, "get_report: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_report: Optimize has not run");
  *report = o->report;
  return PHOVO_OK;
}

int phovo_odometry_get_trust_region_report(const phovo_odometry *o, phovo_trust_region_report *report)
{
  if (!o || !report) return fail(PHOVO_E_INVALID_ARGUMENT, "get_trust_region_report: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_trust_region_report: Optimize has not run");
  if (!o->have_tr_report) return fail(PHOVO_E_UNSUPPORTED, "get_trust_region_report: the last Optimize ran under another objective");
  *report = o->tr_report;
  return PHOVO_OK;
}

int phovo_odometry_get_pair_system(const phovo_odometry *o, phovo_pair_system *out)
{
  if (!o || !out) return fail(PHOVO_E_INVALID_ARGUMENT, "get_pair_system: null");
  if (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL)
    return fail(PHOVO_E_UNSUPPORTED, "get_pair_system: the inverse-compositional objective has its system in "
                                     "phovo_odometry_get_inverse_system");
  if (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST)
    return fail(PHOVO_E_UNSUPPORTED, "get_pair_system: the robust inverse-compositional objective has its system in "
                                     "phovo_odometry_get_robust_system");
  if (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE)
    return fail(PHOVO_E_UNSUPPORTED, "get_pair_system: the semi-dense inverse-compositional objective has no system yet");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_pair_system: Optimize has not run since the frames were set");
  const phovo_engine *e = o->engine;
  int finest = -1;                                        // the lowest level Optimize() iterates on
  for (int l = e->cfg.num_levels - 1; l >= 0; l--)
    if (e->cfg.max_num_iterations[l] > 0) finest = l;
  if (finest < 0) return fail(PHOVO_E_NOT_READY, "get_pair_system: the configuration optimises no level");
  const int src = 0, tgt = 1;
  return phovo_engine_evaluate_pairs(o->engine, 1, &src, &tgt, o->state, finest, out);
}

int phovo_odometry_get_sampled_system(const phovo_odometry *o, phovo_sampled_system *out)
{
  if (!o || !out) return fail(PHOVO_E_INVALID_ARGUMENT, "get_sampled_system: null");
  if (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL)
    return fail(PHOVO_E_UNSUPPORTED, "get_sampled_system: the inverse-compositional objective has its system in "
                                     "phovo_odometry_get_inverse_system");
  if (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST)
    return fail(PHOVO_E_UNSUPPORTED, "get_sampled_system: the robust inverse-compositional objective has its system in "
                                     "phovo_odometry_get_robust_system");
  if (o->engine->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE)
    return fail(PHOVO_E_UNSUPPORTED, "get_sampled_system: the semi-dense inverse-compositional objective has no system yet");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_sampled_system: Optimize has not run since the frames were set");
  const phovo_engine *e = o->engine;
  int finest = -1;                                        // the lowest level Optimize() iterates on
  for (int l = e->cfg.num_levels - 1; l >= 0; l--)
    if (e->cfg.max_num_iterations[l] > 0) finest = l;
  if (finest < 0) return fail(PHOVO_E_NOT_READY, "get_sampled_system: the configuration optimises no level");
  const int src = 0, tgt = 1;
  double state[8];
  std::memcpy(state, o->state, sizeof(double) * 6);
  const bool affine = o->have_illumination && e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE;
  state[6] = affine ? o->illumination[0] : 0.0;
  state[7] = affine ? o->illumination[1] : 0.0;
  return phovo_engine_evaluate_sampled_pairs(o->engine, 1, &src, &tgt, state,
                                             e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE ? 8 : 6, finest, out);
}

int phovo_odometry_get_geometric_system(const phovo_odometry *o, phovo_geometric_system *out)
{
  if (!o || !out) return fail(PHOVO_E_INVALID_ARGUMENT, "get_geometric_system: null");
  const phovo_engine *e = o->engine;
  if (e->objective != PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
    return fail(PHOVO_E_UNSUPPORTED, "get_geometric_system: the photometric-geometric objective only");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_geometric_system: Optimize has not run since the frames were set");
  int finest = -1;                                        // the lowest level Optimize() iterates on
  for (int l = e->cfg.num_levels - 1; l >= 0; l--)
    if (e->cfg.max_num_iterations[l] > 0) finest = l;
  if (finest < 0) return fail(PHOVO_E_NOT_READY, "get_geometric_system: the configuration optimises no level");
  const int src = 0, tgt = 1;
  return phovo_engine_evaluate_geometric_pairs(o->engine, 1, &src, &tgt, o->state, finest, out);
}

int phovo_odometry_get_objective_system(const phovo_odometry *o, phovo_pair_system *out)
{
  if (!o || !out) return fail(PHOVO_E_INVALID_ARGUMENT, "get_objective_system: null");
  const phovo_engine *e = o->engine;
  if (e->objective != PHOVO_OBJECTIVE_TRUST_REGION && e->objective != PHOVO_OBJECTIVE_BIOBJECTIVE)
    return fail(PHOVO_E_UNSUPPORTED, "get_objective_system: the trust-region and the bi-objective objective only (the others "
                                     "have phovo_odometry_get_pair_system, _get_sampled_system and _get_geometric_system)");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_objective_system: Optimize has not run since the frames were set");
  int finest = -1;                                        // the lowest level Optimize() iterates on
  for (int l = e->cfg.num_levels - 1; l >= 0; l--)
    if (e->cfg.max_num_iterations[l] > 0) finest = l;
  if (finest < 0) return fail(PHOVO_E_NOT_READY, "get_objective_system: the configuration optimises no level");
  const int src = 0, tgt = 1;
  return phovo_engine_evaluate_objective_pairs(o->engine, 1, &src, &tgt, o->state, finest, out);
}

int phovo_odometry_get_inverse_system(const phovo_odometry *o, phovo_pair_system *out)
{
  if (!o || !out) return fail(PHOVO_E_INVALID_ARGUMENT, "get_inverse_system: null");
  const phovo_engine *e = o->engine;
  if (e->objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL)
    return fail(PHOVO_E_UNSUPPORTED, "get_inverse_system: the inverse-compositional objective only (the others have "
                                     "phovo_odometry_get_pair_system, _get_sampled_system, _get_geometric_system and "
                                     "_get_objective_system)");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_inverse_system: Optimize has not run since the frames were set");
  int finest = -1;                                        // the lowest level Optimize() iterates on
  for (int l = e->cfg.num_levels - 1; l >= 0; l--)
    if (e->cfg.max_num_iterations[l] > 0) finest = l;
  if (finest < 0) return fail(PHOVO_E_NOT_READY, "get_inverse_system: the configuration optimises no level");
  const int src = 0, tgt = 1;
  return phovo_engine_evaluate_inverse_pairs(o->engine, 1, &src, &tgt, o->state, finest, out);
}

int phovo_odometry_get_robust_system(const phovo_odometry *o, phovo_robust_system *out)
{
  if (!o || !out) return fail(PHOVO_E_INVALID_ARGUMENT, "get_robust_system: null");
  const phovo_engine *e = o->engine;
  if (e->objective != PHOVO_OBJECTIVE_INVERSE_ROBUST)
    return fail(PHOVO_E_UNSUPPORTED, "get_robust_system: the robust inverse-compositional objective only (the others have "
                                     "phovo_odometry_get_pair_system, _get_sampled_system, _get_geometric_system, "
                                     "_get_objective_system and _get_inverse_system)");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "get_robust_system: Optimize has not run since the frames were set");
  int finest = -1;                                        // the lowest level Optimize() iterates on
  for (int l = e->cfg.num_levels - 1; l >= 0; l--)
    if (e->cfg.max_num_iterations[l] > 0) finest = l;
  if (finest < 0) return fail(PHOVO_E_NOT_READY, "get_robust_system: the configuration optimises no level");
  const int src = 0, tgt = 1;
  return phovo_engine_evaluate_robust_pairs(o->engine, 1, &src, &tgt, o->state, nullptr, finest, out);
}

int phovo_odometry_last_optimize_ms(const phovo_odometry *o, double *ms)
{
  if (!o || !ms) return fail(PHOVO_E_INVALID_ARGUMENT, "last_optimize_ms: null");
  if (!o->optimized) return fail(PHOVO_E_NOT_READY, "last_optimize_ms: Optimize has not run");
  return phovo_engine_last_align_ms(o->engine, ms, nullptr);
}

}  // extern "C"
