// PhotoconsistencyVisualOdometry on the MI355X path: frame-to-frame odometry over a TUM-format RGB-D
// directory, writing a TUM trajectory file.
//
//   ./PhotoconsistencyVisualOdometry <config_file.yml> <rgbd_dataset_directory> <output_trajectory_file> [--batch [--gpus N] [--rccl]]
//                                    [--method analytic|ceres|biobjective|inverse|robust|semidense|affine|geometric] [--information <file>] [--system <file>]
//                                    [--geometric-system <file>] [--objective-system <file>] [--inverse-system <file>]
//                                    [--robust-system <file>] [--prior-weight <wt>,<wr>] [--min-pixel-gradient <g>[,<g>...]]
// --method picks the aligner as the reference's USE_PHOTOCONSISTENCY_ODOMETRY_METHOD does (0 = analytic, the default;
// 1 = ceres: Levenberg-Marquardt on bilinear samples, CPhotoconsistencyOdometryCeres, which reads config_*_ceres.yml
// files; 2 = bi-objective: photometric and depth error together, CPhotoconsistencyOdometryBiObjective), in every mode;
// affine is not in the reference: the photometric aligner with a per-pair gain and offset, CPhotoconsistencyOdometryAffine,
// which reads the analytic files.
// geometric is not in the reference either: intensity and depth rows together on the bilinear samples,
// CPhotoconsistencyOdometryGeometric, which reads the analytic files and their optional depth_weight / max_depth_residual keys.
// inverse is not in the reference either: the photometric residual aligned inverse-compositionally (the Jacobian from the
// source frame's own gradient, the step composed on SE(3)), CPhotoconsistencyOdometryInverse, which reads the analytic files;
// its system is in the twist basis, so the four Euler-basis system flags below refuse it and --inverse-system writes it.
// robust is not in the reference either: the inverse-compositional aligner under a Huber weight whose threshold follows the
// median of the pair's own residuals, CPhotoconsistencyOdometryRobust, which reads the analytic files; its system carries
// the weights, so the five older system flags below refuse it and --robust-system writes it.
// A configuration file of the other kind is refused with a message that says so.
// --information <file> (not in the reference; analytic method, one device): one line per pair, stamped like its trajectory
// line, with the Gauss-Newton system at the pair's optimal state on the finest level the configuration optimises --
// `timestamp rows cost` and the 21 upper-triangle entries of J^T J (phovo_pair_system_format).  The loop takes it from the
// class surface (GetPairSystem), --batch from phovo_engine_evaluate_pairs; both write the same bytes, and the trajectory
// file is the same with and without the flag.  The printed times do not include the evaluation.
// --system <file> (not in the reference; one device): the same for the aligners that sample the target bilinearly -- --method
// affine, and --method analytic when the yml sets sampling_bilinear: 1 (which --batch then honours like the loop, with the
// file's other extension keys).  One line per pair, `timestamp rows cost dim` and the dim (dim + 1) / 2 upper-triangle
// entries of J^T W J (phovo_sampled_system_format; dim 8 under affine: pose, alpha, beta).  The loop takes it from the class
// surface (GetSampledSystem), --batch from phovo_engine_evaluate_sampled_pairs (alpha and beta from
// phovo_engine_fetch_illumination); both write the same bytes, and the trajectory file is the same with and without the flag.
// --geometric-system <file> (not in the reference; --method geometric, one device): the same for that method -- one line per
// pair, `timestamp rows depth_rows photometric_cost depth_cost`, the 21 upper-triangle entries of the photometric block
// sum J_I J_I^T and the 21 of the depth block sum J_D J_D^T (phovo_geometric_system_format; the system the aligner solves is
// their entry-by-entry sum).  The loop takes it from the class surface (GetGeometricSystem), --batch from
// phovo_engine_evaluate_geometric_pairs; both write the same bytes, the trajectory file is the same with and without the
// flag, and the printed times do not include the evaluation.
// --objective-system <file> (not in the reference; --method ceres or biobjective, one device): the same for the reference's
// methods 1 and 2 -- one line per pair, `timestamp rows cost` and the 21 upper-triangle entries of J^T J
// (phovo_pair_system_format) at the pair's optimal state on the finest optimised level; under ceres cost is r^T r, twice
// the solver's final cost.  The loop takes it from the class surface (GetObjectiveSystem), --batch from
// phovo_engine_evaluate_objective_pairs; both write the same bytes, the trajectory file is the same with and without the
// flag, and the printed times do not include the evaluation.
// --inverse-system <file> (not in the reference; --method inverse, one device): the same for the inverse-compositional
// method -- one line per pair, `timestamp rows cost` and the 21 upper-triangle entries of sum J J^T
// (phovo_pair_system_format) at the pair's optimal state on the finest optimised level, in the TWIST basis (nu, omega) of
// the right-hand perturbation T Exp(xi): xi lives in the source camera's frame (include/phovo_hip.h,
// phovo_engine_evaluate_inverse_pairs).  The loop takes it from the class surface (GetInverseSystem), --batch from
// phovo_engine_evaluate_inverse_pairs; both write the same bytes, the trajectory file is the same with and without the
// flag, and the printed times do not include the evaluation.
// semidense is not in the reference either: the inverse-compositional aligner on the source pixels whose gradient magnitude
// reaches a per-level threshold, CPhotoconsistencyOdometrySemiDense, which reads the analytic files and their optional key
// `min_pixel_gradient (at each level)`; it has no system yet, so every system flag below refuses it.
// --min-pixel-gradient <g>[,<g>...] (--method semidense, the loop and --batch): that threshold from the command line, one
// value for all levels or one per level, each finite and >= 0, in place of the file's.
// --prior-weight <wt>,<wr> (not in the reference; --method inverse | robust, the pair-by-pair loop): a constant-velocity
// Gaussian prior on every pair's pose (include/phovo_hip.h, phovo_prior_options) -- the prior pose is the
// previous pair's result, zero for the first pair, and Lambda = diag(wt, wt, wt, wr, wr, wr) in the twist order (nu, omega);
// every pair's record (phovo_prior_report_format) goes to the standard output.  Refused with --batch, where no pair knows the
// one before it, and under the other methods.  With 0,0 the trajectory file is the one without the flag, byte for byte.
// --robust-system <file> (not in the reference; --method robust, one device): the same for the robust method -- one line per
// pair, `timestamp rows outliers delta median cost huber_cost squared_cost`, the 6 entries of sum w J r and the 21
// upper-triangle entries of sum w J J^T (phovo_robust_system_format) at the pair's optimal state on the finest optimised
// level, with the Huber threshold taken from the median of the residuals at that state, in the twist basis of
// --inverse-system (include/phovo_hip.h, phovo_engine_evaluate_robust_pairs).  The loop takes it from the class surface
// (GetRobustSystem), --batch from phovo_engine_evaluate_robust_pairs; both write the same bytes, the trajectory file is the
// same with and without the flag, and the printed times do not include the evaluation.
//
// Behaviour kept from the reference's app (apps/PhotoconsistencyVisualOdometry/PhotoconsistencyVisualOdometry.cpp):
//   * <dir>/rgb.txt and <dir>/depth.txt are read in lock step -- line n of one is paired with line n of the
//     other, there is NO timestamp association (phovo/include/CMultiSensorDataSource.h:74-91); '#' lines are
//     skipped and image paths are relative to the list file (CCameraRecord.h:74-108);
//   * intrinsics (517.3, 516.5, 318.6, 255.3) and depth scale 1/5000 are hard-coded (:163,170-173);
//   * every pair starts from the zero state (:175,224) -> pairs are independent;
//   * pose *= Rt^-1, quaternion from the rotation block, one line `timestamp tx ty tz qx qy qz qw` with 16
//     significant digits per pair, stamped with the CURRENT rgb timestamp (:233-243).
// Default mode goes pair by pair through the class surface exactly like the reference's loop and prints
// `Time = ... sec.` and `Rt:` for each.  --batch loads the whole sequence, builds every pyramid once on the
// GPU (the reference builds each frame's pyramids twice, :222-223) and aligns all pairs in one batched call;
// the trajectory is identical.  --batch --gpus N cuts the pairs into N contiguous ranges, one engine and one host thread
// per device (single process: the results meet in host memory; with --rccl through ONE RCCL all_gather from the engines'
// device buffers, apps/rccl/rccl_gather.cpp); the trajectory file is the same for every N and either way.  The
// one-process-per-GPU form with the RCCL all_gather is apps/PhotoconsistencyVisualOdometrySharded.py.
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "io/png_io.h"
#include "rccl/rccl_gather.h"
#include "rccl/shard_vote.h"
#include "phovo/CPhotoconsistencyOdometryAnalytic.h"
#include "phovo/CPhotoconsistencyOdometryAffine.h"
#include "phovo/CPhotoconsistencyOdometryInverse.h"
#include "phovo/CPhotoconsistencyOdometryRobust.h"
#include "phovo/CPhotoconsistencyOdometrySemiDense.h"
#include "min_pixel_gradient.h"
#include "phovo/CPhotoconsistencyOdometryGeometric.h"
#include "phovo/CPhotoconsistencyOdometryBiObjective.h"
#include "phovo/CPhotoconsistencyOdometryCeres.h"

typedef double CoordinateType;
typedef unsigned char PixelType;
typedef phovo::Numeric::Matrix33RowMajor<CoordinateType> Matrix33Type;
typedef phovo::Numeric::Matrix44RowMajor<CoordinateType> Matrix44Type;
typedef phovo::Numeric::VectorCol6<CoordinateType> Vector6Type;
typedef phovo::compat::Mat_<PixelType> IntensityImageType;
typedef phovo::compat::Mat_<CoordinateType> DepthImageType;

struct ListEntry { double timestamp; std::string path; };

static bool fileExists(const std::string &p) { struct stat st; return ::stat(p.c_str(), &st) == 0; }

static std::string parentDir(const std::string &p)
{
  const size_t s = p.find_last_of('/');
  return s == std::string::npos ? std::string(".") : p.substr(0, s);
}

static bool readList(const std::string &listFile, std::vector<ListEntry> &out)
{
  std::ifstream in(listFile.c_str());
  if (!in.is_open()) { std::cerr << "Unable to open camera record file " << listFile << std::endl; return false; }
  const std::string dir = parentDir(listFile);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream iss(line);
    ListEntry e;
    std::string name;
    if (!(iss >> e.timestamp >> name)) continue;
    e.path = dir + "/" + name;
    out.push_back(e);
  }
  return true;
}

static bool loadGray(const std::string &path, IntensityImageType &img)
{
  phovo_io::Image8 im; std::string err;
  if (!phovo_io::read_gray8(path, &im, &err)) { std::cerr << err << std::endl; return false; }
  img.create(im.height, im.width);
  for (size_t i = 0; i < im.pixels.size(); i++) img.data[i] = im.pixels[i];
  return true;
}

static bool loadDepth16(const std::string &path, phovo_io::Image16 &im)
{
  std::string err;
  if (!phovo_io::read_unchanged16(path, &im, &err)) { std::cerr << err << std::endl; return false; }
  return true;
}

// pose chain and trajectory line live behind the C ABI (phovo_trajectory_*): this loop, the --batch path and the
// multi-rank sequence driver write byte-identical files
static bool writePose(std::ofstream &f, double timestamp, const Matrix44Type &pose)
{
  char line[256];
  if (phovo_trajectory_format_pose(timestamp, pose.data(), line, sizeof(line)) != PHOVO_OK) return false;
  f << line << std::endl;                                                    // :240-243
  return true;
}

static bool writeSystem(std::ofstream &f, double timestamp, const phovo_pair_system &s)
{
  char line[1024];
  if (phovo_pair_system_format(timestamp, &s, line, sizeof(line)) != PHOVO_OK) return false;
  f << line << std::endl;
  return true;
}

static bool writeSystem(std::ofstream &f, double timestamp, const phovo_robust_system &s)
{
  char line[1024];
  if (phovo_robust_system_format(timestamp, &s, line, sizeof(line)) != PHOVO_OK) return false;
  f << line << std::endl;
  return true;
}

static bool writeSystem(std::ofstream &f, double timestamp, const phovo_sampled_system &s)
{
  char line[1024];
  if (phovo_sampled_system_format(timestamp, &s, line, sizeof(line)) != PHOVO_OK) return false;
  f << line << std::endl;
  return true;
}

static bool writeSystem(std::ofstream &f, double timestamp, const phovo_geometric_system &s)
{
  char line[PHOVO_GEOMETRIC_SYSTEM_LINE_CAPACITY];
  if (phovo_geometric_system_format(timestamp, &s, line, sizeof(line)) != PHOVO_OK) return false;
  f << line << std::endl;
  return true;
}

// GetGeometricSystem() of the class that has one (the loop is one generic lambda over every --method's class; the flag is
// refused before the loop for the others)
template <class Odometry>
static auto geometricSystemOf(Odometry &odometry, int) -> decltype(odometry.GetGeometricSystem())
{
  return odometry.GetGeometricSystem();
}
template <class Odometry>
static phovo_geometric_system geometricSystemOf(Odometry &, long)
{
  throw std::runtime_error("--geometric-system needs --method geometric");
}

// GetObjectiveSystem() of the classes that have one, in the same way.
template <class Odometry>
static auto objectiveSystemOf(Odometry &odometry, int) -> decltype(odometry.GetObjectiveSystem())
{
  return odometry.GetObjectiveSystem();
}
template <class Odometry>
static phovo_pair_system objectiveSystemOf(Odometry &, long)
{
  throw std::runtime_error("--objective-system needs --method ceres or --method biobjective");
}

// GetInverseSystem() of the class that has one, in the same way.
template <class Odometry>
static auto inverseSystemOf(Odometry &odometry, int) -> decltype(odometry.GetInverseSystem())
{
  return odometry.GetInverseSystem();
}
template <class Odometry>
static phovo_pair_system inverseSystemOf(Odometry &, long)
{
  throw std::runtime_error("--inverse-system needs --method inverse");
}

// GetRobustSystem() of the class that has one, in the same way.
template <class Odometry>
static auto robustSystemOf(Odometry &odometry, int) -> decltype(odometry.GetRobustSystem())
{
  return odometry.GetRobustSystem();
}
template <class Odometry>
static phovo_robust_system robustSystemOf(Odometry &, long)
{
  throw std::runtime_error("--robust-system needs --method robust");
}

// SetPosePrior() / GetPriorReport() of the classes that have them, in the same way.
template <class Odometry>
static auto setPosePriorOf(Odometry &odometry, const double *state, const double *information, int)
    -> decltype(odometry.SetPosePrior(state, information), void())
{
  odometry.SetPosePrior(state, information);
}
template <class Odometry>
static void setPosePriorOf(Odometry &, const double *, const double *, long)
{
  throw std::runtime_error("--prior-weight needs --method inverse or --method robust");
}
template <class Odometry>
static auto priorReportOf(Odometry &odometry, int) -> decltype(odometry.GetPriorReport())
{
  return odometry.GetPriorReport();
}
template <class Odometry>
static phovo_prior_report priorReportOf(Odometry &, long)
{
  throw std::runtime_error("--prior-weight needs --method inverse or --method robust");
}

static void printHelp()
{
  std::cout << "./PhotoconsistencyVisualOdometry <config_file.yml> <rgbd_dataset_directory> "
               "<output_trajectory_file> [--batch [--gpus N] [--rccl]] [--method analytic|ceres|biobjective|inverse|robust|semidense|affine|geometric] "
               "[--information <file>] [--system <file>] [--geometric-system <file>] [--objective-system <file>] "
               "[--inverse-system <file>] [--robust-system <file>] [--min-pixel-gradient <g>[,<g>...]] "
               "[--prior-weight <wt>,<wr>]" << std::endl;
}

#define PHOVO_OK_OR_FAIL(call)                                                              \
  do { if ((call) != PHOVO_OK) { std::cerr << #call << ": " << phovo_last_error() << std::endl; return EXIT_FAILURE; } } while (0)

int main(int argc, char *argv[])
{
  if (argc < 4) { printHelp(); return EXIT_FAILURE; }
  const std::string configFile(argv[1]), datasetDir(argv[2]), trajectoryPath(argv[3]);
  bool batch = false;
  int nGpus = 1;                                      // --batch --gpus N: the pairs of the sequence sharded over N devices
  bool rccl = false;                                  // ... --rccl: the shards' states meet through ONE RCCL all_gather
  int objective = PHOVO_OBJECTIVE_PHOTOMETRIC;        // --method analytic (default) | ceres | biobjective
  std::string informationPath;                        // --information <file>: the pairs' systems at their optimal states
  std::string systemPath;                             // --system <file>: the same for the sampled aligners
  std::string geometricSystemPath;                    // --geometric-system <file>: the same for --method geometric
  std::string objectiveSystemPath;                    // --objective-system <file>: the same for --method ceres | biobjective
  std::string inverseSystemPath;                      // --inverse-system <file>: the same for --method inverse (twist basis)
  std::string robustSystemPath;                       // --robust-system <file>: the same for --method robust (weighted, twist basis)
  bool priorWeight = false;                           // --prior-weight <wt>,<wr>: a constant-velocity pose prior (loop mode)
  double priorWt = 0.0, priorWr = 0.0;
  std::vector<double> minPixelGradient;               // --min-pixel-gradient <g>[,<g>...]: --method semidense's thresholds
  for (int i = 4; i < argc; i++) {
    const std::string a(argv[i]);
    if (a == "--batch") batch = true;
    else if (a == "--prior-weight" && i + 1 < argc) {
      const char *text = argv[++i];
      char *end = nullptr;
      priorWt = std::strtod(text, &end);
      const bool comma = end != text && *end == ',';
      const char *second = comma ? end + 1 : end;
      priorWr = comma ? std::strtod(second, &end) : 0.0;
      if (!comma || end == second || *end != '\0' || !std::isfinite(priorWt) || !std::isfinite(priorWr) || priorWt < 0.0 || priorWr < 0.0) {
        std::cerr << "--prior-weight needs <wt>,<wr>: two finite numbers >= 0" << std::endl;
        return EXIT_FAILURE;
      }
      priorWeight = true;
    }
    else if (a == "--method" && i + 1 < argc) {
      const std::string m(argv[++i]);
      if (m == "analytic") objective = PHOVO_OBJECTIVE_PHOTOMETRIC;
      else if (m == "biobjective") objective = PHOVO_OBJECTIVE_BIOBJECTIVE;
      else if (m == "ceres") objective = PHOVO_OBJECTIVE_TRUST_REGION;
      else if (m == "affine") objective = PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE;
      else if (m == "geometric") objective = PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC;
      else if (m == "inverse") objective = PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL;
      else if (m == "robust") objective = PHOVO_OBJECTIVE_INVERSE_ROBUST;
      else if (m == "semidense") objective = PHOVO_OBJECTIVE_INVERSE_SEMIDENSE;
      else { printHelp(); return EXIT_FAILURE; }
    }
    else if (a == "--min-pixel-gradient" && i + 1 < argc) {
      if (!phovo_apps::parseMinPixelGradient(argv[++i], minPixelGradient)) {
        std::cerr << "--min-pixel-gradient needs <g>[,<g>...]: one value for all levels or one per level, each finite and >= 0" << std::endl;
        return EXIT_FAILURE;
      }
    }
    else if (a == "--rccl") rccl = true;
    else if (a == "--gpus" && i + 1 < argc) nGpus = std::atoi(argv[++i]);
    else if (a == "--information" && i + 1 < argc) informationPath = argv[++i];
    else if (a == "--system" && i + 1 < argc) systemPath = argv[++i];
    else if (a == "--geometric-system" && i + 1 < argc) geometricSystemPath = argv[++i];
    else if (a == "--objective-system" && i + 1 < argc) objectiveSystemPath = argv[++i];
    else if (a == "--inverse-system" && i + 1 < argc) inverseSystemPath = argv[++i];
    else if (a == "--robust-system" && i + 1 < argc) robustSystemPath = argv[++i];
    else { printHelp(); return EXIT_FAILURE; }
  }
  if (nGpus < 1 || (nGpus > 1 && !batch)) { std::cerr << "--gpus N needs --batch and N >= 1" << std::endl; return EXIT_FAILURE; }
  if (rccl && !batch) { std::cerr << "--rccl needs --batch" << std::endl; return EXIT_FAILURE; }
  const bool information = !informationPath.empty();
  if (information && (nGpus > 1 || rccl)) {
    std::cerr << "--information runs on one device: it cannot be combined with --gpus N > 1 or --rccl" << std::endl;
    return EXIT_FAILURE;
  }
  if (information && objective != PHOVO_OBJECTIVE_PHOTOMETRIC) {
    std::cerr << "--information needs --method analytic (the bi-objective and the Ceres method have no pair system there: "
                 "--objective-system writes theirs)" << std::endl;
    return EXIT_FAILURE;
  }
  const bool sampled = !systemPath.empty();
  if (sampled && (nGpus > 1 || rccl)) {
    std::cerr << "--system runs on one device: it cannot be combined with --gpus N > 1 or --rccl" << std::endl;
    return EXIT_FAILURE;
  }
  if (sampled && objective != PHOVO_OBJECTIVE_PHOTOMETRIC && objective != PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE) {
    std::cerr << "--system needs bilinear sampling or --method affine" << std::endl;
    return EXIT_FAILURE;
  }
  const bool geometricSystem = !geometricSystemPath.empty();
  if (geometricSystem && (nGpus > 1 || rccl)) {
    std::cerr << "--geometric-system runs on one device: it cannot be combined with --gpus N > 1 or --rccl" << std::endl;
    return EXIT_FAILURE;
  }
  if (geometricSystem && objective != PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) {
    std::cerr << "--geometric-system needs --method geometric" << std::endl;
    return EXIT_FAILURE;
  }
  const bool objectiveSystem = !objectiveSystemPath.empty();
  if (objectiveSystem && (nGpus > 1 || rccl)) {
    std::cerr << "--objective-system runs on one device: it cannot be combined with --gpus N > 1 or --rccl" << std::endl;
    return EXIT_FAILURE;
  }
  if (objectiveSystem && objective != PHOVO_OBJECTIVE_TRUST_REGION && objective != PHOVO_OBJECTIVE_BIOBJECTIVE) {
    std::cerr << "--objective-system needs --method ceres or --method biobjective" << std::endl;
    return EXIT_FAILURE;
  }
  const bool inverseSystem = !inverseSystemPath.empty();
  if (inverseSystem && (nGpus > 1 || rccl)) {
    std::cerr << "--inverse-system runs on one device: it cannot be combined with --gpus N > 1 or --rccl" << std::endl;
    return EXIT_FAILURE;
  }
  if (inverseSystem && objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL) {
    std::cerr << "--inverse-system needs --method inverse" << std::endl;
    return EXIT_FAILURE;
  }
  const bool robustSystem = !robustSystemPath.empty();
  if (robustSystem && (nGpus > 1 || rccl)) {
    std::cerr << "--robust-system runs on one device: it cannot be combined with --gpus N > 1 or --rccl" << std::endl;
    return EXIT_FAILURE;
  }
  if (robustSystem && objective != PHOVO_OBJECTIVE_INVERSE_ROBUST) {
    std::cerr << "--robust-system needs --method robust" << std::endl;
    return EXIT_FAILURE;
  }
  if (!minPixelGradient.empty() && objective != PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {
    std::cerr << "--min-pixel-gradient needs --method semidense" << std::endl;
    return EXIT_FAILURE;
  }
  if (priorWeight && batch) {
    std::cerr << "--prior-weight runs pair by pair (the prior is the previous pair's result): it cannot be combined with --batch" << std::endl;
    return EXIT_FAILURE;
  }
  if (priorWeight && objective != PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL && objective != PHOVO_OBJECTIVE_INVERSE_ROBUST) {
    std::cerr << "--prior-weight needs --method inverse or --method robust" << std::endl;
    return EXIT_FAILURE;
  }
  if (!fileExists(configFile)) { std::cerr << "Input config file " << configFile << " does not exist" << std::endl; return EXIT_FAILURE; }
  {   // the Ceres method reads the config_*_ceres.yml keys, the other two the config_*_analytic.yml keys
    phovo_config c;
    phovo_trust_region_options o;
    const bool ceres = objective == PHOVO_OBJECTIVE_TRUST_REGION;
    if ((ceres ? phovo_trust_region_read_file(configFile.c_str(), &c, &o) : phovo_config_read_file(configFile.c_str(), &c)) != PHOVO_OK) {
      std::cerr << configFile << " is not a configuration file for --method " << (ceres ? "ceres" : "analytic|biobjective")
                << " (" << phovo_last_error() << "): --method ceres reads the config_*_ceres.yml files, the other methods "
                << "the config_*_analytic.yml files" << std::endl;
      return EXIT_FAILURE;
    }
  }
  // --method analytic: the extension keys of the file (sampling_bilinear, jacobian_corrected, ...), which the class reads
  // in ReadConfigurationFile and --batch hands to its engines
  phovo_extensions extensions;
  PHOVO_OK_OR_FAIL(phovo_extensions_default(&extensions));
  if (objective == PHOVO_OBJECTIVE_PHOTOMETRIC) PHOVO_OK_OR_FAIL(phovo_extensions_read_file(configFile.c_str(), &extensions));
  if (sampled && objective == PHOVO_OBJECTIVE_PHOTOMETRIC && extensions.sampling != PHOVO_SAMPLING_BILINEAR) {
    std::cerr << "--system needs bilinear sampling or --method affine" << std::endl;
    return EXIT_FAILURE;
  }
  if (!fileExists(datasetDir)) { std::cerr << "Input RGBD dataset directory " << datasetDir << " does not exist" << std::endl; return EXIT_FAILURE; }
  const std::string rgbList = datasetDir + "/rgb.txt", depthList = datasetDir + "/depth.txt";
  if (!fileExists(rgbList)) { std::cerr << "Input RGB data file " << rgbList << " does not exist" << std::endl; return EXIT_FAILURE; }
  if (!fileExists(depthList)) { std::cerr << "Input depth data file " << depthList << " does not exist" << std::endl; return EXIT_FAILURE; }
  const std::string outDir = parentDir(trajectoryPath);
  if (!fileExists(outDir) && ::mkdir(outDir.c_str(), 0777) != 0) {
    std::cerr << "Cannot create output directory " << outDir << std::endl;
    return EXIT_FAILURE;
  }

  const CoordinateType depthScalingFactor = 1. / 5000.;                    // :163
  Matrix33Type intrinsicMatrix;                                              // :170-173
  intrinsicMatrix << 517.3, 0., 318.6,
                     0., 516.5, 255.3,
                     0., 0., 1.;

  std::vector<ListEntry> rgb, depth;
  if (!readList(rgbList, rgb) || !readList(depthList, depth)) return EXIT_FAILURE;
  const size_t nFrames = rgb.size() < depth.size() ? rgb.size() : depth.size();   // lock step: stops at the shorter list

  std::ofstream trajectoryFile(trajectoryPath.c_str());
  if (!trajectoryFile.is_open()) { std::cerr << "Cannot open output trajectory file " << trajectoryPath << std::endl; return EXIT_FAILURE; }
  trajectoryFile << "# estimated trajectory" << std::endl;                    // :187-188
  trajectoryFile << "# timestamp tx ty tz qx qy qz qw" << std::endl;
  std::ofstream informationFile;
  if (information) {
    informationFile.open(informationPath.c_str());
    if (!informationFile.is_open()) { std::cerr << "Cannot open output information file " << informationPath << std::endl; return EXIT_FAILURE; }
  }
  std::ofstream systemFile;
  if (sampled) {
    systemFile.open(systemPath.c_str());
    if (!systemFile.is_open()) { std::cerr << "Cannot open output system file " << systemPath << std::endl; return EXIT_FAILURE; }
  }
  std::ofstream geometricSystemFile;
  if (geometricSystem) {
    geometricSystemFile.open(geometricSystemPath.c_str());
    if (!geometricSystemFile.is_open()) { std::cerr << "Cannot open output geometric system file " << geometricSystemPath << std::endl; return EXIT_FAILURE; }
  }
  std::ofstream objectiveSystemFile;
  if (objectiveSystem) {
    objectiveSystemFile.open(objectiveSystemPath.c_str());
    if (!objectiveSystemFile.is_open()) { std::cerr << "Cannot open output objective system file " << objectiveSystemPath << std::endl; return EXIT_FAILURE; }
  }
  std::ofstream inverseSystemFile;
  if (inverseSystem) {
    inverseSystemFile.open(inverseSystemPath.c_str());
    if (!inverseSystemFile.is_open()) { std::cerr << "Cannot open output inverse system file " << inverseSystemPath << std::endl; return EXIT_FAILURE; }
  }
  std::ofstream robustSystemFile;
  if (robustSystem) {
    robustSystemFile.open(robustSystemPath.c_str());
    if (!robustSystemFile.is_open()) { std::cerr << "Cannot open output robust system file " << robustSystemPath << std::endl; return EXIT_FAILURE; }
  }
  if (nFrames < 2) return EXIT_SUCCESS;

  Matrix44Type pose = Matrix44Type::Identity();
  try {
    // the pair-by-pair loop through the class surface, with the class --method names
    auto runLoop = [&](auto &odometry) -> int {
      odometry.ReadConfigurationFile(configFile);
      phovo_apps::applyMinPixelGradient(odometry, minPixelGradient, 0);
      odometry.SetIntrinsicMatrix(intrinsicMatrix);
      IntensityImageType prevGray, curGray;
      DepthImageType prevDepth, curDepth;
      phovo_io::Image16 d16;
      if (!loadGray(rgb[0].path, prevGray) || !loadDepth16(depth[0].path, d16)) return EXIT_FAILURE;
      prevDepth.create(d16.height, d16.width);
      for (size_t i = 0; i < d16.pixels.size(); i++) prevDepth.data[i] = (double)d16.pixels[i] * depthScalingFactor;
      Vector6Type priorState = Vector6Type::Zero();                          // --prior-weight: the previous pair's result
      double priorInformation[36] = {};
      for (int d = 0; d < 6; d++) priorInformation[7 * d] = d < 3 ? priorWt : priorWr;
      for (size_t t = 1; t < nFrames; t++) {
        if (!loadGray(rgb[t].path, curGray) || !loadDepth16(depth[t].path, d16)) return EXIT_FAILURE;
        curDepth.create(d16.height, d16.width);
        for (size_t i = 0; i < d16.pixels.size(); i++) curDepth.data[i] = (double)d16.pixels[i] * depthScalingFactor;

        odometry.SetSourceFrame(prevGray, prevDepth);                        // :222-224
        odometry.SetTargetFrame(curGray, curDepth);
        odometry.SetInitialStateVector(Vector6Type::Zero());
        if (priorWeight) setPosePriorOf(odometry, priorState.data(), priorInformation, 0);
        const auto t0 = std::chrono::steady_clock::now();
        odometry.Optimize();
        const auto t1 = std::chrono::steady_clock::now();
        std::cout << "Time = " << std::chrono::duration<double>(t1 - t0).count() << " sec." << std::endl;

        const Matrix44Type Rt = odometry.GetOptimalRigidTransformationMatrix();
        const Vector6Type state = odometry.GetOptimalStateVector();
        if (priorWeight) {
          const phovo_prior_report report = priorReportOf(odometry, 0);
          char line[256];
          PHOVO_OK_OR_FAIL(phovo_prior_report_format(rgb[t].timestamp, &report, line, sizeof(line)));
          std::cout << "Prior: " << line << std::endl;
          priorState = state;
        }
        PHOVO_OK_OR_FAIL(phovo_trajectory_chain(1, state.data(), pose.data(), nullptr));   // pose *= Rt^-1  :233-234
        if (!writePose(trajectoryFile, rgb[t].timestamp, pose)) return EXIT_FAILURE;
        if (information && !writeSystem(informationFile, rgb[t].timestamp, odometry.GetPairSystem())) return EXIT_FAILURE;
        if (sampled && !writeSystem(systemFile, rgb[t].timestamp, odometry.GetSampledSystem())) return EXIT_FAILURE;
        if (geometricSystem && !writeSystem(geometricSystemFile, rgb[t].timestamp, geometricSystemOf(odometry, 0))) return EXIT_FAILURE;
        if (objectiveSystem && !writeSystem(objectiveSystemFile, rgb[t].timestamp, objectiveSystemOf(odometry, 0))) return EXIT_FAILURE;
        if (inverseSystem && !writeSystem(inverseSystemFile, rgb[t].timestamp, inverseSystemOf(odometry, 0))) return EXIT_FAILURE;
        if (robustSystem && !writeSystem(robustSystemFile, rgb[t].timestamp, robustSystemOf(odometry, 0))) return EXIT_FAILURE;
        std::cout << "Rt:" << std::endl << Rt << std::endl;
        prevGray = curGray.clone();
        prevDepth = curDepth.clone();
      }
      return EXIT_SUCCESS;
    };
    if (!batch) {
      if (objective == PHOVO_OBJECTIVE_BIOBJECTIVE) {
        phovo::Analytic::CPhotoconsistencyOdometryBiObjective<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      } else if (objective == PHOVO_OBJECTIVE_TRUST_REGION) {
        phovo::Ceres::CPhotoconsistencyOdometryCeres<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      } else if (objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE) {
        phovo::Analytic::CPhotoconsistencyOdometryAffine<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      } else if (objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC) {
        phovo::Analytic::CPhotoconsistencyOdometryGeometric<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      } else if (objective == PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL) {
        phovo::Analytic::CPhotoconsistencyOdometryInverse<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      } else if (objective == PHOVO_OBJECTIVE_INVERSE_ROBUST) {
        phovo::Analytic::CPhotoconsistencyOdometryRobust<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      } else if (objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {
        phovo::Analytic::CPhotoconsistencyOdometrySemiDense<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      } else {
        phovo::Analytic::CPhotoconsistencyOdometryAnalytic<PixelType, CoordinateType> odometry;
        if (runLoop(odometry) != EXIT_SUCCESS) return EXIT_FAILURE;
      }
    } else {
      phovo_config cfg;
      phovo_trust_region_options trOptions;           // --method ceres: the solver options of the file
      if (objective == PHOVO_OBJECTIVE_TRUST_REGION)
        PHOVO_OK_OR_FAIL(phovo_trust_region_read_file(configFile.c_str(), &cfg, &trOptions));
      else
        PHOVO_OK_OR_FAIL(phovo_config_read_file(configFile.c_str(), &cfg));
      phovo_geometric_options geoOptions;             // --method geometric: the two optional keys of the file
      PHOVO_OK_OR_FAIL(phovo_geometric_options_default(&geoOptions));
      if (objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC)
        PHOVO_OK_OR_FAIL(phovo_geometric_read_file(configFile.c_str(), &geoOptions));
      phovo_semidense_options sdOptions;              // --method semidense: the optional key of the file, then the command line
      PHOVO_OK_OR_FAIL(phovo_semidense_options_default(&sdOptions));
      if (objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE) {
        PHOVO_OK_OR_FAIL(phovo_semidense_read_file(configFile.c_str(), &sdOptions));
        phovo_apps::overrideMinPixelGradient(minPixelGradient, sdOptions);
      }
      const int nDevices = phovo_device_count();
      if (nDevices < 1) { std::cerr << "phovo_engine_create: no HIP device available: this library has no CPU path" << std::endl; return EXIT_FAILURE; }
      // PHOVO_VO_SHARE_DEVICES=1 lets more shards than devices run (a rehearsal of --gpus N on a smaller machine)
      if (nGpus > nDevices && !std::getenv("PHOVO_VO_SHARE_DEVICES")) {
        std::cerr << "--gpus " << nGpus << " but only " << nDevices << " device(s) are visible" << std::endl;
        return EXIT_FAILURE;
      }
      // Decoding is the bulk of this mode's wall time (a 640x480 colour PNG + its 16-bit depth PNG take 6-20 ms on one
      // core, the alignment of the whole sequence a few milliseconds on the GPU): frames are independent, so they
      // are decoded by all host threads at once, each straight into its slot of the two packed arrays.
      IntensityImageType gray;
      phovo_io::Image16 d16;
      std::vector<uint8_t> allGray;
      std::vector<uint16_t> allDepth;
      if (!loadGray(rgb[0].path, gray) || !loadDepth16(depth[0].path, d16)) return EXIT_FAILURE;
      const int W = gray.cols, H = gray.rows;
      if (d16.width != W || d16.height != H) { std::cerr << "frame 0: intensity and depth sizes differ" << std::endl; return EXIT_FAILURE; }
      allGray.resize((size_t)W * H * nFrames);
      allDepth.resize((size_t)W * H * nFrames);
      std::copy(gray.data, gray.data + (size_t)W * H, allGray.begin());
      std::copy(d16.pixels.begin(), d16.pixels.end(), allDepth.begin());
      {
        unsigned nThreads = std::thread::hardware_concurrency();
        if (nThreads == 0) nThreads = 1;
        if (nThreads > 32) nThreads = 32;
        if ((size_t)nThreads > nFrames) nThreads = (unsigned)nFrames;
        std::atomic<size_t> next(1);
        std::atomic<long> failed(-1);
        std::vector<std::string> errors(nThreads);
        auto worker = [&](unsigned id) {
          phovo_io::Image8 g8;
          phovo_io::Image16 g16;
          for (;;) {
            const size_t t = next.fetch_add(1);
            if (t >= nFrames || failed.load() >= 0) return;
            std::string err;
            if (!phovo_io::read_gray8(rgb[t].path, &g8, &err) || !phovo_io::read_unchanged16(depth[t].path, &g16, &err)) {
              errors[id] = err; failed.store((long)t); return;
            }
            if (g8.width != W || g8.height != H || g16.width != W || g16.height != H) {
              errors[id] = "frame " + std::to_string(t) + " has a different size"; failed.store((long)t); return;
            }
            std::copy(g8.pixels.begin(), g8.pixels.end(), allGray.begin() + (size_t)W * H * t);
            std::copy(g16.pixels.begin(), g16.pixels.end(), allDepth.begin() + (size_t)W * H * t);
          }
        };
        std::vector<std::thread> pool;
        for (unsigned id = 0; id < nThreads; id++) pool.emplace_back(worker, id);
        for (auto &th : pool) th.join();
        if (failed.load() >= 0) {
          for (const auto &e : errors) if (!e.empty()) std::cerr << e << std::endl;
          return EXIT_FAILURE;
        }
      }
      // Pair t aligns frame t with frame t+1 and depends on nothing else (:175,222-224): the pairs are cut into nGpus
      // contiguous ranges (the first nPairs % nGpus ranges one pair longer), each range gets its own engine on its own
      // device and its own host thread, and needs the frames of its range plus one.  In ONE process the results meet
      // in host memory: no collective (the multi-process form, PhotoconsistencyVisualOdometrySharded.py, is where the
      // RCCL all_gather is).  With phovo_engine_set_batch_invariant a pair's result does not depend on its batch, so the file is the same for every N.
      const int nPairs = (int)nFrames - 1;
      std::vector<double> states((size_t)nPairs * 6);
      std::vector<phovo_pair_system> systems(information ? (size_t)nPairs : 0);
      int finestLevel = -1;                             // --information: the lowest level the configuration optimises
      for (int l = cfg.num_levels - 1; l >= 0; l--)
        if (cfg.max_num_iterations[l] > 0) finestLevel = l;
      if (information && finestLevel < 0) { std::cerr << "--information: the configuration optimises no level" << std::endl; return EXIT_FAILURE; }
      if (sampled && finestLevel < 0) { std::cerr << "--system: the configuration optimises no level" << std::endl; return EXIT_FAILURE; }
      if (geometricSystem && finestLevel < 0) { std::cerr << "--geometric-system: the configuration optimises no level" << std::endl; return EXIT_FAILURE; }
      if (objectiveSystem && finestLevel < 0) { std::cerr << "--objective-system: the configuration optimises no level" << std::endl; return EXIT_FAILURE; }
      if (inverseSystem && finestLevel < 0) { std::cerr << "--inverse-system: the configuration optimises no level" << std::endl; return EXIT_FAILURE; }
      std::vector<phovo_pair_system> inverseSystems(inverseSystem ? (size_t)nPairs : 0);
      if (robustSystem && finestLevel < 0) { std::cerr << "--robust-system: the configuration optimises no level" << std::endl; return EXIT_FAILURE; }
      std::vector<phovo_robust_system> robustSystems(robustSystem ? (size_t)nPairs : 0);
      std::vector<phovo_pair_system> objectiveSystems(objectiveSystem ? (size_t)nPairs : 0);
      std::vector<phovo_geometric_system> geometricSystems(geometricSystem ? (size_t)nPairs : 0);
      const int systemDim = objective == PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE ? 8 : 6;
      std::vector<phovo_sampled_system> sampledSystems(sampled ? (size_t)nPairs : 0);
      std::vector<std::string> shardError(nGpus);
      // --rccl: instead of every shard copying its states to the host itself, the shards' device buffers meet in ONE RCCL
      // all_gather (one communicator and one host thread per device in this one process) and rank 0 copies the lot out --
      // the collective of SURVEY.md section 8e, with the host side staying C++.  Same bytes in the trajectory file.
      phovo_rccl::Group group;
      const int maxShard = nPairs / nGpus + (nPairs % nGpus ? 1 : 0);
      if (rccl) {
        std::vector<int> devices(nGpus);
        for (int g = 0; g < nGpus; g++) devices[g] = g % nDevices;
        std::string err;
        if (!group.create(devices, &err)) { std::cerr << err << std::endl; return EXIT_FAILURE; }
      }
      const auto t0 = std::chrono::steady_clock::now();
      std::chrono::steady_clock::time_point tAligned{};     // --information (one shard): when the alignment had ended
      // Every shard thread arrives at the vote exactly once -- also one that failed on its way there, and one whose range
      // is empty -- and the collective is entered only if all of them are ready for it: a rank that stays away from an
      // all_gather leaves the others waiting in it for ever.
      phovo_rccl::ShardVote vote(nGpus);
      // test hook: shard N reports a failure before it touches its device (tests: the run must end with that error, not hang)
      const int injectFailure = std::getenv("PHOVO_VO_INJECT_SHARD_FAILURE") ? std::atoi(std::getenv("PHOVO_VO_INJECT_SHARD_FAILURE")) : -1;
      auto alignShard = [&](int g) {
        const int base = nPairs / nGpus, extra = nPairs % nGpus;
        const int a = g * base + (g < extra ? g : extra), b = a + base + (g < extra ? 1 : 0);
        const int f0 = a, nf = b - a + 1;
        phovo_engine *engine = nullptr;
        void *dStates = nullptr;
        auto work = [&]() -> bool {                       // everything of this shard short of the collective
          auto fail = [&](const char *what) { shardError[g] = std::string(what) + ": " + phovo_last_error(); return false; };
          if (b <= a) return true;                        // more shards than pairs: nothing to align, still a rank of the gather
          if (injectFailure == g) { shardError[g] = "shard " + std::to_string(g) + ": failure injected (PHOVO_VO_INJECT_SHARD_FAILURE)"; return false; }
          if (phovo_engine_create(g % nDevices, &engine) != PHOVO_OK) return fail("phovo_engine_create");
          if (phovo_engine_set_config(engine, &cfg) != PHOVO_OK) return fail("phovo_engine_set_config");
          if (phovo_engine_set_objective(engine, objective) != PHOVO_OK) return fail("phovo_engine_set_objective");
          if (objective == PHOVO_OBJECTIVE_PHOTOMETRIC && phovo_engine_set_extensions(engine, &extensions) != PHOVO_OK)
            return fail("phovo_engine_set_extensions");
          if (objective == PHOVO_OBJECTIVE_INVERSE_SEMIDENSE && phovo_engine_set_semidense_options(engine, &sdOptions) != PHOVO_OK)
            return fail("phovo_engine_set_semidense_options");
          if (objective == PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC && phovo_engine_set_geometric_options(engine, &geoOptions) != PHOVO_OK)
            return fail("phovo_engine_set_geometric_options");
          if (objective == PHOVO_OBJECTIVE_TRUST_REGION && phovo_engine_set_trust_region_options(engine, &trOptions) != PHOVO_OK)
            return fail("phovo_engine_set_trust_region_options");
          // a pair's pose must not depend on the size of the shard it falls into (same trajectory file for every N)
          if (phovo_engine_set_batch_invariant(engine, 1) != PHOVO_OK) return fail("phovo_engine_set_batch_invariant");
          if (phovo_engine_set_intrinsic_matrix(engine, intrinsicMatrix.data()) != PHOVO_OK) return fail("phovo_engine_set_intrinsic_matrix");
          if (phovo_engine_reserve_frames(engine, nf, W, H) != PHOVO_OK) return fail("phovo_engine_reserve_frames");
          if (phovo_engine_upload_frames_u16(engine, 0, nf, PHOVO_ROLE_BOTH, allGray.data() + (size_t)W * H * f0, (size_t)W,
                                             (size_t)W * H, allDepth.data() + (size_t)W * H * f0, sizeof(uint16_t) * (size_t)W,
                                             sizeof(uint16_t) * (size_t)W * H, depthScalingFactor) != PHOVO_OK)
            return fail("phovo_engine_upload_frames_u16");
          std::vector<int> src(b - a), tgt(b - a);
          for (int p = 0; p < b - a; p++) { src[p] = p; tgt[p] = p + 1; }
          if (!rccl) {
            if (phovo_engine_align_pairs(engine, b - a, src.data(), tgt.data(), nullptr, states.data() + (size_t)a * 6, nullptr) != PHOVO_OK)
              return fail("phovo_engine_align_pairs");
            if (information || sampled || geometricSystem || objectiveSystem || inverseSystem || robustSystem)
              tAligned = std::chrono::steady_clock::now();                    // (the evaluation is not part of the timed run)
            if (robustSystem && phovo_engine_evaluate_robust_pairs(engine, b - a, src.data(), tgt.data(), states.data() + (size_t)a * 6,
                                                                   nullptr, finestLevel, robustSystems.data() + a) != PHOVO_OK)
              return fail("phovo_engine_evaluate_robust_pairs");
            if (inverseSystem && phovo_engine_evaluate_inverse_pairs(engine, b - a, src.data(), tgt.data(), states.data() + (size_t)a * 6,
                                                                     finestLevel, inverseSystems.data() + a) != PHOVO_OK)
              return fail("phovo_engine_evaluate_inverse_pairs");
            if (objectiveSystem && phovo_engine_evaluate_objective_pairs(engine, b - a, src.data(), tgt.data(), states.data() + (size_t)a * 6,
                                                                         finestLevel, objectiveSystems.data() + a) != PHOVO_OK)
              return fail("phovo_engine_evaluate_objective_pairs");
            if (geometricSystem && phovo_engine_evaluate_geometric_pairs(engine, b - a, src.data(), tgt.data(), states.data() + (size_t)a * 6,
                                                                         finestLevel, geometricSystems.data() + a) != PHOVO_OK)
              return fail("phovo_engine_evaluate_geometric_pairs");
            if (information && phovo_engine_evaluate_pairs(engine, b - a, src.data(), tgt.data(), states.data() + (size_t)a * 6,
                                                           finestLevel, systems.data() + a) != PHOVO_OK)
              return fail("phovo_engine_evaluate_pairs");
            if (sampled) {                                // the states the systems are evaluated at: [pairs][6], or [pairs][8] with alpha, beta
              const int n = b - a;
              std::vector<double> at((size_t)n * systemDim), illum((size_t)n * 2);
              if (systemDim == 8 && phovo_engine_fetch_illumination(engine, n, illum.data()) != PHOVO_OK)
                return fail("phovo_engine_fetch_illumination");
              for (int p = 0; p < n; p++) {
                std::copy(states.begin() + (size_t)(a + p) * 6, states.begin() + (size_t)(a + p) * 6 + 6, at.begin() + (size_t)p * systemDim);
                if (systemDim == 8) { at[(size_t)p * 8 + 6] = illum[(size_t)p * 2]; at[(size_t)p * 8 + 7] = illum[(size_t)p * 2 + 1]; }
              }
              if (phovo_engine_evaluate_sampled_pairs(engine, n, src.data(), tgt.data(), at.data(), systemDim, finestLevel,
                                                      sampledSystems.data() + a) != PHOVO_OK)
                return fail("phovo_engine_evaluate_sampled_pairs");
            }
            return true;
          }
          if (phovo_engine_enqueue_align(engine, b - a, src.data(), tgt.data(), nullptr) != PHOVO_OK) return fail("phovo_engine_enqueue_align");
          if (phovo_engine_synchronize(engine) != PHOVO_OK) return fail("phovo_engine_synchronize");
          if (phovo_engine_results_device_ptr(engine, &dStates) != PHOVO_OK) return fail("phovo_engine_results_device_ptr");
          return true;
        };
        bool ok = work();
        if (rccl) {
          std::string err;
          if (ok && !group.stage(g, dStates, b > a ? b - a : 0, maxShard, &err)) { shardError[g] = err; ok = false; }
          if (vote.arrive(ok)) {                          // every rank is staged: all of them enter the collective
            if (!group.gather(g, &err)) shardError[g] = err;
          } else if (ok) {
            shardError[g] = "";                           // (another shard failed and says so; this one just stays out)
          }
        }
        if (engine) phovo_engine_destroy(engine);
      };
      {
        std::vector<std::thread> shards;
        for (int g = 1; g < nGpus; g++) shards.emplace_back(alignShard, g);
        alignShard(0);
        for (auto &th : shards) th.join();
      }
      for (const auto &e : shardError) if (!e.empty()) { std::cerr << e << std::endl; return EXIT_FAILURE; }
      if (rccl) {                          // rank 0's view of the gather: shard g's block holds its (b - a) x 6 states
        for (int g = 0; g < nGpus; g++) {
          const int base = nPairs / nGpus, extra = nPairs % nGpus;
          const int a = g * base + (g < extra ? g : extra), b = a + base + (g < extra ? 1 : 0);
          std::copy(group.gathered(g), group.gathered(g) + (size_t)(b - a) * 6, states.begin() + (size_t)a * 6);
        }
      }
      const auto t1 = (information || sampled || geometricSystem || objectiveSystem || inverseSystem || robustSystem) ? tAligned : std::chrono::steady_clock::now();
      std::cout << "Time = " << std::chrono::duration<double>(t1 - t0).count() << " sec. (" << nPairs << " pairs on " << nGpus
                << " device(s), upload and pyramids included)" << std::endl;
      std::vector<double> poses((size_t)nPairs * 16);
      PHOVO_OK_OR_FAIL(phovo_trajectory_chain(nPairs, states.data(), pose.data(), poses.data()));
      for (int p = 0; p < nPairs; p++) {
        Matrix44Type P;
        for (int i = 0; i < 16; i++) P(i) = poses[(size_t)p * 16 + i];
        if (!writePose(trajectoryFile, rgb[(size_t)p + 1].timestamp, P)) return EXIT_FAILURE;
        if (information && !writeSystem(informationFile, rgb[(size_t)p + 1].timestamp, systems[(size_t)p])) return EXIT_FAILURE;
        if (sampled && !writeSystem(systemFile, rgb[(size_t)p + 1].timestamp, sampledSystems[(size_t)p])) return EXIT_FAILURE;
        if (geometricSystem && !writeSystem(geometricSystemFile, rgb[(size_t)p + 1].timestamp, geometricSystems[(size_t)p])) return EXIT_FAILURE;
        if (objectiveSystem && !writeSystem(objectiveSystemFile, rgb[(size_t)p + 1].timestamp, objectiveSystems[(size_t)p])) return EXIT_FAILURE;
        if (inverseSystem && !writeSystem(inverseSystemFile, rgb[(size_t)p + 1].timestamp, inverseSystems[(size_t)p])) return EXIT_FAILURE;
        if (robustSystem && !writeSystem(robustSystemFile, rgb[(size_t)p + 1].timestamp, robustSystems[(size_t)p])) return EXIT_FAILURE;
      }
    }
  } catch (const std::exception &e) {
    std::cerr << "error: " << e.what() << std::endl;
    return EXIT_FAILURE;
  }
  trajectoryFile.close();
  if (information) informationFile.close();
  if (sampled) systemFile.close();
  if (geometricSystem) geometricSystemFile.close();
  if (objectiveSystem) objectiveSystemFile.close();
  if (inverseSystem) inverseSystemFile.close();
  if (robustSystem) robustSystemFile.close();
  return EXIT_SUCCESS;
}
