// The Gauss-Newton systems at given poses behind the C ABI (include/phovo_hip.h): phovo_engine_evaluate_pairs,
// _evaluate_sampled_pairs, _evaluate_geometric_pairs, _evaluate_objective_pairs, _evaluate_inverse_pairs and
// _evaluate_robust_pairs.  Each entry point keeps what is its own -- the objectives and
// samplings it refuses, its state width, its workspace regions, the extras of its args and its launch -- and shares the
// rest: the refusals about the call, the one workspace, and the loop over groups of pairs.

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "engine_internal.hpp"

using namespace phovo_hip;

namespace {

// Owner maps of one evaluation group take at most this much: 218 pairs at 640x480.
constexpr size_t EVAL_OWNER_CAP_BYTES = (size_t)256 << 20;
// Tile sums of one sampled-evaluation group take at most this much: 436 pairs of eight columns (873 of six, and of the
// inverse-compositional call) at 640x480.
constexpr size_t EVAL_SAMPLED_SLAB_CAP_BYTES = (size_t)64 << 20;
// Tile sums of one geometric-evaluation group (the sampled and the depth slab together) take at most this much: 436 pairs
// at 640x480.
constexpr size_t EVAL_GEOMETRIC_SLAB_CAP_BYTES = (size_t)64 << 20;

// The pairs of one group: as many as the call has, as long as `per_pair` bytes of each stay within `cap`; at least one.
int eval_group(int n_pairs, size_t cap, size_t per_pair)
{
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)n_pairs, cap / per_pair));
}

struct EvalCall {                    // an entry point's name in its refusals, and what its caller passed
  const char *name;
  int n_pairs;
  const int *src, *tgt;
  const double *states;
  int state_dim;
  int level;
  void *out;
  size_t out_size;                   // of one result record
};

// Everything the entry points refuse alike, behind their own refusals of objectives and samplings.  A call of no pairs is
// valid once its arguments are: it returns PHOVO_OK before the pool is looked at.  `target_depth`: the launch reads the
// target's depth plane too.  `source_gradients`: it reads the source's gradient planes too (engine_align.cpp's rule for the
// inverse-compositional objective).  On PHOVO_OK with pairs, every enqueue in flight has finished (their slots are not
// touched).
int eval_check(phovo_engine *e, const EvalCall &c, bool target_depth, bool source_gradients = false)
{
  const std::string who = c.name;
  if (c.n_pairs < 0) return fail(PHOVO_E_INVALID_ARGUMENT, who + ": n_pairs < 0");
  if (c.n_pairs > 0 && (!c.src || !c.tgt || !c.states || !c.out)) return fail(PHOVO_E_INVALID_ARGUMENT, who + ": null");
  if (c.level < 0 || c.level >= e->cfg.num_levels) return fail(PHOVO_E_INVALID_ARGUMENT, who + ": level out of range");
  if (c.n_pairs == 0) return PHOVO_OK;
  if (e->n_frames == 0) return fail(PHOVO_E_NOT_READY, who + ": no frames uploaded");
  for (int i = 0; i < c.n_pairs; i++) {
    if (c.src[i] < 0 || c.src[i] >= e->n_frames || c.tgt[i] < 0 || c.tgt[i] >= e->n_frames)
      return fail(PHOVO_E_INVALID_ARGUMENT, who + ": frame index out of range");
  }
  if (!e->have_K) return fail(PHOVO_E_NOT_READY, who + ": SetIntrinsicMatrix has not been called");
  if (!e->levels[c.level].stored) return fail(PHOVO_E_NOT_READY, who + ": the level is not resident (phovo_engine_level_is_stored)");
  for (int i = 0; i < c.n_pairs; i++) {
    if (!(e->frame_roles[(size_t)c.src[i] * PHOVO_MAX_LEVELS + (size_t)c.level] & PHOVO_ROLE_SOURCE))
      return fail(PHOVO_E_NOT_READY, who + ": a source frame has no depth (upload it with PHOVO_ROLE_SOURCE)");
    if (!(e->frame_roles[(size_t)c.tgt[i] * PHOVO_MAX_LEVELS + (size_t)c.level] & PHOVO_ROLE_TARGET))
      return fail(PHOVO_E_NOT_READY, who + ": a target frame has no gradients (upload it with PHOVO_ROLE_TARGET)");
    if (target_depth && !(e->frame_roles[(size_t)c.tgt[i] * PHOVO_MAX_LEVELS + (size_t)c.level] & PHOVO_ROLE_SOURCE))
      return fail(PHOVO_E_NOT_READY, who + ": the photometric-geometric objective reads the target's depth "
                                           "(upload target frames with PHOVO_ROLE_BOTH)");
    if (source_gradients && !(e->frame_roles[(size_t)c.src[i] * PHOVO_MAX_LEVELS + (size_t)c.level] & PHOVO_ROLE_TARGET))
      return fail(PHOVO_E_NOT_READY, who + ": the inverse-compositional objective reads the source's gradient planes "
                                           "(upload source frames with PHOVO_ROLE_BOTH)");
  }
  PHOVO_HIP_CHECK(hipSetDevice(e->device));
  PHOVO_HIP_CHECK(quiesce(e));                 // behind every enqueue in flight; their slots are not touched
  return PHOVO_OK;
}

// The engine's evaluation workspace, grown where it is too small, cut into regions of bytes[i] bytes in this order, every
// one 256-byte aligned: at[i] is where region i starts.  `owner_ints`: the leading ints of region 0 that are owner maps and
// so must hold -1 (0: region 0 holds something else).  The watermark of what is known to hold -1 falls to 0 HERE, for every
// call: whoever leaves owner maps at -1 behind raises it again when its call has ended without an error.
template <size_t N>
int eval_workspace(phovo_engine *e, const size_t (&bytes)[N], unsigned char *(&at)[N], size_t owner_ints)
{
  size_t need = 0;
  for (size_t b : bytes) need += (b + 255) & ~(size_t)255;
  const size_t clean = need <= e->eval_ws.capacity ? e->eval_owner_clean : 0;      // (a new allocation holds anything)
  PHOVO_HIP_CHECK(e->eval_ws.reserve(need));
  e->eval_owner_clean = 0;
  size_t off = 0;
  for (size_t i = 0; i < N; i++) {
    at[i] = e->eval_ws.ptr + off;
    off += (bytes[i] + 255) & ~(size_t)255;
  }
  // pass 2 restores the -1 it covers, but the regions behind an earlier, smaller owner area may hold ballots or sums of that
  // call, and the front the tile sums of a sampled or geometric one
  if (owner_ints > clean) PHOVO_HIP_CHECK(fill_i32(reinterpret_cast<int *>(at[0]), owner_ints, -1, e->stream));
  return PHOVO_OK;
}

// The level's view and where the group's states and pair indices lie: in[0..2], three regions of the workspace.
template <class Args>
void eval_args(Args &a, const phovo_engine *e, int level, unsigned char *const *in)
{
  fill_level_view(a, e, level);
  a.states = reinterpret_cast<const double *>(in[0]);
  a.src = reinterpret_cast<const int *>(in[1]);
  a.tgt = reinterpret_cast<const int *>(in[2]);
}

// The call's pairs in groups of `group`, one after the other: states and pair indices to in[0..2], launch(pairs of the
// group), the records at d_out back to the caller.
template <class Launch>
int eval_run(phovo_engine *e, const EvalCall &c, int group, unsigned char *const *in, const void *d_out, Launch launch)
{
  const size_t dim = (size_t)c.state_dim;
  for (int g0 = 0; g0 < c.n_pairs; g0 += group) {
    const int n = std::min(group, c.n_pairs - g0);
    PHOVO_HIP_CHECK(hipMemcpyAsync(in[0], c.states + (size_t)g0 * dim, sizeof(double) * dim * (size_t)n, hipMemcpyHostToDevice, e->stream));
    PHOVO_HIP_CHECK(hipMemcpyAsync(in[1], c.src + g0, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    PHOVO_HIP_CHECK(hipMemcpyAsync(in[2], c.tgt + g0, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    PHOVO_HIP_CHECK(launch(n));
    PHOVO_HIP_CHECK(hipMemcpyAsync(static_cast<char *>(c.out) + c.out_size * (size_t)g0, d_out, c.out_size * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    PHOVO_HIP_CHECK(hipStreamSynchronize(e->stream));      // (the next group's inputs overwrite this one's)
  }
  return PHOVO_OK;
}

}  // namespace

extern "C" {

int phovo_engine_evaluate_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt, const double *states,
                                int level, phovo_pair_system *out)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "evaluate_pairs: null engine");
  if (e->objective != PHOVO_OBJECTIVE_PHOTOMETRIC)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_pairs: the bi-objective, the trust-region and the affine-illumination objective "
                                     "have no pair system here (photometric objective only; the inverse-compositional "
                                     "objective has phovo_engine_evaluate_inverse_pairs)");
  if (e->ext.sampling != PHOVO_SAMPLING_NEAREST_SCATTER)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_pairs: bilinear sampling has no pair system here (nearest / scatter only)");
  const EvalCall c{"evaluate_pairs", n_pairs, src, tgt, states, 6, level, out, sizeof(*out)};
  int st = eval_check(e, c, false);
  if (st != PHOVO_OK || n_pairs == 0) return st;

  // Workspace for a group of G pairs: owner maps first (kept at -1 between calls), then ballots, tile sums, states, pair
  // indices and the results.
  const int n_level = e->levels[level].n;
  const size_t n = (size_t)n_level, n_chunks = (n + 63) / 64;
  const int group = eval_group(n_pairs, EVAL_OWNER_CAP_BYTES, n * sizeof(int));
  const size_t G = (size_t)group;
  const size_t bytes[] = {G * n * sizeof(int), G * n_chunks * sizeof(unsigned long long),
                          G * gn_eval_slab_doubles_per_pair(n_level) * sizeof(double),
                          G * 6 * sizeof(double), G * sizeof(int), G * sizeof(int), G * sizeof(phovo_pair_system)};
  unsigned char *at[7];
  st = eval_workspace(e, bytes, at, G * n);
  if (st != PHOVO_OK) return st;

  GNEvalArgs a{};
  eval_args(a, e, level, at + 3);
  a.huber_delta = e->ext.huber_delta[level];
  auto *d_owner = reinterpret_cast<int *>(at[0]);
  auto *d_mask = reinterpret_cast<unsigned long long *>(at[1]);
  auto *d_part = reinterpret_cast<double *>(at[2]);
  auto *d_out = reinterpret_cast<phovo_pair_system *>(at[6]);
  st = eval_run(e, c, group, at + 3, d_out, [&](int pairs) {
    return gn_eval_pairs(a, pairs, e->ext.plane_storage, d_owner, d_mask, d_part, d_out, e->stream);
  });
  if (st == PHOVO_OK) e->eval_owner_clean = G * n;         // pass 2 has put every owner map back to -1
  return st;
}

int phovo_engine_evaluate_sampled_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt, const double *states,
                                        int state_dim, int level, phovo_sampled_system *out)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "evaluate_sampled_pairs: null engine");
  if (e->objective == PHOVO_OBJECTIVE_BIOBJECTIVE || e->objective == PHOVO_OBJECTIVE_TRUST_REGION)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_sampled_pairs: the bi-objective and the trust-region objective have no sampled "
                                     "system (bilinear sampling or the affine-illumination objective only)");
  if (e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_sampled_pairs: the photometric-geometric objective has no sampled system");
  if (e->objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_sampled_pairs: the inverse-compositional objective has its system in "
                                     "phovo_engine_evaluate_inverse_pairs");
  if (e->objective == PHOVO_OBJECTIVE_INVERSE_ROBUST)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_sampled_pairs: the robust inverse-compositional objective has its system in "
                                     "phovo_engine_evaluate_robust_pairs");
  if (e->objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_sampled_pairs: the semi-dense inverse-compositional objective has no system yet");
  const bool affine = e->objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE;
  if (!affine && e->ext.sampling != PHOVO_SAMPLING_BILINEAR)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_sampled_pairs: nearest / scatter sampling has its system in "
                                     "phovo_engine_evaluate_pairs (bilinear sampling or the affine-illumination objective only)");
  const int dim = affine ? 8 : 6;
  if (state_dim != dim)
    return fail(PHOVO_E_INVALID_ARGUMENT, affine ? "evaluate_sampled_pairs: the affine-illumination objective takes state_dim 8"
                                                 : "evaluate_sampled_pairs: bilinear sampling takes state_dim 6");
  const EvalCall c{"evaluate_sampled_pairs", n_pairs, src, tgt, states, dim, level, out, sizeof(*out)};
  int st = eval_check(e, c, false);
  if (st != PHOVO_OK || n_pairs == 0) return st;

  // Workspace for a group of G pairs: tile sums, states, pair indices and the results.
  const size_t slab_bytes = gn_eval_sampled_slab_doubles_per_pair(e->levels[level].n, dim) * sizeof(double);
  const int group = eval_group(n_pairs, EVAL_SAMPLED_SLAB_CAP_BYTES, slab_bytes);
  const size_t G = (size_t)group;
  const size_t bytes[] = {G * slab_bytes, G * (size_t)dim * sizeof(double), G * sizeof(int), G * sizeof(int),
                          G * sizeof(phovo_sampled_system)};
  unsigned char *at[5];
  st = eval_workspace(e, bytes, at, 0);
  if (st != PHOVO_OK) return st;

  GNSampledEvalArgs a{};
  eval_args(a, e, level, at + 1);
  a.state_dim = dim;
  a.huber_delta = affine ? 0.0 : e->ext.huber_delta[level];
  const bool corrected = affine || e->ext.jacobian_corrected != 0;
  auto *d_part = reinterpret_cast<double *>(at[0]);
  auto *d_out = reinterpret_cast<phovo_sampled_system *>(at[4]);
  return eval_run(e, c, group, at + 1, d_out, [&](int pairs) {
    return gn_eval_sampled_pairs(a, pairs, e->ext.plane_storage, corrected, d_part, d_out, e->stream);
  });
}

int phovo_engine_evaluate_geometric_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt, const double *states,
                                          int level, phovo_geometric_system *out)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "evaluate_geometric_pairs: null engine");
  if (e->objective != PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_geometric_pairs: the photometric-geometric objective only (the "
                                     "inverse-compositional objective has phovo_engine_evaluate_inverse_pairs)");
  // (set_objective / set_extensions hold this objective to fp64 planes without Huber weights)
  const EvalCall c{"evaluate_geometric_pairs", n_pairs, src, tgt, states, 6, level, out, sizeof(*out)};
  int st = eval_check(e, c, true);
  if (st != PHOVO_OK || n_pairs == 0) return st;

  // Workspace for a group of G pairs: the sampled tile sums, the depth tile sums, states, pair indices, the sampled records
  // and the results.  One group size serves both launches.
  const size_t slab_bytes = gn_eval_sampled_slab_doubles_per_pair(e->levels[level].n, 6) * sizeof(double);
  const int group = eval_group(n_pairs, EVAL_GEOMETRIC_SLAB_CAP_BYTES, 2 * slab_bytes);
  const size_t G = (size_t)group;
  const size_t bytes[] = {G * slab_bytes, G * slab_bytes, G * 6 * sizeof(double), G * sizeof(int), G * sizeof(int),
                          G * sizeof(phovo_sampled_system), G * sizeof(phovo_geometric_system)};
  unsigned char *at[7];
  st = eval_workspace(e, bytes, at, 0);
  if (st != PHOVO_OK) return st;

  GNGeometricEvalArgs b{};
  eval_args(b.s, e, level, at + 2);
  b.s.state_dim = 6;
  b.s.huber_delta = 0.0;
  b.depth_weight = e->geo_opt.depth_weight[level];
  b.max_depth_residual = e->geo_opt.max_depth_residual[level];
  auto *d_part_sampled = reinterpret_cast<double *>(at[0]);
  auto *d_part_depth = reinterpret_cast<double *>(at[1]);
  auto *d_sampled = reinterpret_cast<phovo_sampled_system *>(at[5]);
  auto *d_out = reinterpret_cast<phovo_geometric_system *>(at[6]);
  return eval_run(e, c, group, at + 2, d_out, [&](int pairs) {
    return gn_eval_geometric_pairs(b, pairs, d_part_sampled, d_sampled, d_part_depth, d_out, e->stream);
  });
}

int phovo_engine_evaluate_objective_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt, const double *states,
                                          int level, phovo_pair_system *out)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "evaluate_objective_pairs: null engine");
  switch (e->objective) {
    case PHOVO_OBJECTIVE_TRUST_REGION:
    case PHOVO_OBJECTIVE_BIOBJECTIVE:
      break;
    case PHOVO_OBJECTIVE_PHOTOMETRIC:
      return fail(PHOVO_E_UNSUPPORTED, "evaluate_objective_pairs: the photometric objective has its system in "
                                       "phovo_engine_evaluate_pairs (nearest / scatter sampling) or "
                                       "phovo_engine_evaluate_sampled_pairs (bilinear sampling)");
    case PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE:
      return fail(PHOVO_E_UNSUPPORTED, "evaluate_objective_pairs: the affine-illumination objective has its system in "
                                       "phovo_engine_evaluate_sampled_pairs");
    case PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL:
      return fail(PHOVO_E_UNSUPPORTED, "evaluate_objective_pairs: the inverse-compositional objective has its system in "
                                       "phovo_engine_evaluate_inverse_pairs");
    case PHOVO_OBJECTIVE_INVERSE_ROBUST:
      return fail(PHOVO_E_UNSUPPORTED, "evaluate_objective_pairs: the robust inverse-compositional objective has its system in "
                                       "phovo_engine_evaluate_robust_pairs");
    case PHOVO_OBJECTIVE_INVERSE_SEMIDENSE:
      return fail(PHOVO_E_UNSUPPORTED, "evaluate_objective_pairs: the semi-dense inverse-compositional objective has no system yet");
    default:
      return fail(PHOVO_E_UNSUPPORTED, "evaluate_objective_pairs: the photometric-geometric objective has its system in "
                                       "phovo_engine_evaluate_geometric_pairs");
  }
  // (set_objective / set_extensions hold both objectives to fp64 planes, nearest / scatter sampling, no Huber weights; under
  // the bi-objective a target upload carries its depth, so PHOVO_ROLE_TARGET covers the planes the rows read)
  const EvalCall c{"evaluate_objective_pairs", n_pairs, src, tgt, states, 6, level, out, sizeof(*out)};
  int st = eval_check(e, c, false);
  if (st != PHOVO_OK || n_pairs == 0) return st;

  // Workspace for a group of G pairs, as phovo_engine_evaluate_pairs: owner maps first (kept at -1 between calls), then
  // ballots, tile sums, states, pair indices and the results.
  const LevelPool &lv = e->levels[level];
  const size_t n = (size_t)lv.n, n_chunks = (n + 63) / 64;
  const int group = eval_group(n_pairs, EVAL_OWNER_CAP_BYTES, n * sizeof(int));
  const size_t G = (size_t)group;
  const size_t bytes[] = {G * n * sizeof(int), G * n_chunks * sizeof(unsigned long long),
                          G * gn_eval_slab_doubles_per_pair(lv.n) * sizeof(double),
                          G * 6 * sizeof(double), G * sizeof(int), G * sizeof(int), G * sizeof(phovo_pair_system)};
  unsigned char *at[7];
  st = eval_workspace(e, bytes, at, G * n);
  if (st != PHOVO_OK) return st;

  GNObjectiveEvalArgs a{};
  eval_args(a, e, level, at + 3);
  a.dgx_off = lv.dgx_off; a.dgy_off = lv.dgy_off; a.gain_off = lv.gain_off;
  auto *d_owner = reinterpret_cast<int *>(at[0]);
  auto *d_mask = reinterpret_cast<unsigned long long *>(at[1]);
  auto *d_part = reinterpret_cast<double *>(at[2]);
  auto *d_out = reinterpret_cast<phovo_pair_system *>(at[6]);
  st = eval_run(e, c, group, at + 3, d_out, [&](int pairs) {
    return gn_eval_objective_pairs(a, e->objective, pairs, d_owner, d_mask, d_part, d_out, e->stream);
  });
  // the trust region's pass 2 and the bi-objective's fill have put every owner map of every group back to -1
  if (st == PHOVO_OK) e->eval_owner_clean = G * n;
  return st;
}

int phovo_engine_evaluate_inverse_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt, const double *states,
                                        int level, phovo_pair_system *out)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "evaluate_inverse_pairs: null engine");
  if (e->objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_inverse_pairs: the inverse-compositional objective only (the others have "
                                     "phovo_engine_evaluate_pairs, _evaluate_sampled_pairs, _evaluate_geometric_pairs and "
                                     "_evaluate_objective_pairs)");
  // (set_objective / set_extensions hold this objective to fp64 planes without Huber weights)
  const EvalCall c{"evaluate_inverse_pairs", n_pairs, src, tgt, states, 6, level, out, sizeof(*out)};
  int st = eval_check(e, c, false, true);
  if (st != PHOVO_OK || n_pairs == 0) return st;

  // Workspace for a group of G pairs: tile sums, states, pair indices and the results.
  const size_t slab_bytes = gn_eval_slab_doubles_per_pair(e->levels[level].n) * sizeof(double);
  const int group = eval_group(n_pairs, EVAL_SAMPLED_SLAB_CAP_BYTES, slab_bytes);
  const size_t G = (size_t)group;
  const size_t bytes[] = {G * slab_bytes, G * 6 * sizeof(double), G * sizeof(int), G * sizeof(int),
                          G * sizeof(phovo_pair_system)};
  unsigned char *at[5];
  st = eval_workspace(e, bytes, at, 0);
  if (st != PHOVO_OK) return st;

  GNInverseEvalArgs a{};
  eval_args(a, e, level, at + 1);
  auto *d_part = reinterpret_cast<double *>(at[0]);
  auto *d_out = reinterpret_cast<phovo_pair_system *>(at[4]);
  return eval_run(e, c, group, at + 1, d_out, [&](int pairs) {
    return gn_eval_inverse_pairs(a, pairs, d_part, d_out, e->stream);
  });
}

int phovo_engine_evaluate_robust_pairs(phovo_engine *e, int n_pairs, const int *src, const int *tgt, const double *states,
                                       const double *deltas, int level, phovo_robust_system *out)
{
  if (!e) return fail(PHOVO_E_INVALID_ARGUMENT, "evaluate_robust_pairs: null engine");
  if (e->objective != PHOVO_OBJECTIVE_INVERSE_ROBUST)
    return fail(PHOVO_E_UNSUPPORTED, "evaluate_robust_pairs: the robust inverse-compositional objective only (the others have "
                                     "phovo_engine_evaluate_pairs, _evaluate_sampled_pairs, _evaluate_geometric_pairs, "
                                     "_evaluate_objective_pairs and _evaluate_inverse_pairs)");
  // (set_objective / set_extensions hold this objective to fp64 planes without the huber_delta extension)
  const EvalCall c{"evaluate_robust_pairs", n_pairs, src, tgt, states, 6, level, out, sizeof(*out)};
  if (deltas && c.n_pairs >= 0 && src && tgt && states && out) {          // (eval_check refuses the rest below, in its order)
    for (int i = 0; i < n_pairs; i++)
      if (!(deltas[i] > 0.0) || !std::isfinite(deltas[i]))
        return fail(PHOVO_E_INVALID_ARGUMENT, "evaluate_robust_pairs: a delta is not finite and > 0");
  }
  int st = eval_check(e, c, false, true);
  if (st != PHOVO_OK || n_pairs == 0) return st;

  // Workspace for a group of G pairs: tile sums, states, pair indices, the histograms, (m, delta) and the results.
  const size_t slab_bytes = gn_eval_slab_doubles_per_pair(e->levels[level].n) * sizeof(double);
  const size_t hist_bytes = 4096 * sizeof(unsigned), md_bytes = 2 * sizeof(double);
  const int group = eval_group(n_pairs, EVAL_SAMPLED_SLAB_CAP_BYTES, slab_bytes + hist_bytes + md_bytes);
  const size_t G = (size_t)group;
  const size_t bytes[] = {G * slab_bytes, G * 6 * sizeof(double), G * sizeof(int), G * sizeof(int), G * hist_bytes,
                          G * md_bytes, G * sizeof(phovo_robust_system)};
  unsigned char *at[7];
  st = eval_workspace(e, bytes, at, 0);
  if (st != PHOVO_OK) return st;

  GNInverseEvalArgs a{};
  eval_args(a, e, level, at + 1);
  auto *d_part = reinterpret_cast<double *>(at[0]);
  auto *d_hist = reinterpret_cast<unsigned *>(at[4]);
  auto *d_md = reinterpret_cast<double *>(at[5]);
  auto *d_out = reinterpret_cast<phovo_robust_system *>(at[6]);
  // The caller's deltas travel with the states, as (0, delta) per pair: the place the median kernel would have written.
  std::vector<double> md(deltas ? 2 * (size_t)n_pairs : 0);
  for (size_t i = 0; i < md.size() / 2; i++) { md[2 * i] = 0.0; md[2 * i + 1] = deltas[i]; }
  int g0 = 0;                                                             // eval_run's groups come in order
  return eval_run(e, c, group, at + 1, d_out, [&](int pairs) {
    if (deltas) {
      const hipError_t up = hipMemcpyAsync(d_md, md.data() + 2 * (size_t)g0, md_bytes * (size_t)pairs, hipMemcpyHostToDevice, e->stream);
      if (up != hipSuccess) return up;
    }
    g0 += pairs;
    return gn_eval_robust_pairs(a, pairs, e->rob_opt.scale_factor, deltas != nullptr, d_hist, d_md, d_part, d_out, e->stream);
  });
}

}  // extern "C"
