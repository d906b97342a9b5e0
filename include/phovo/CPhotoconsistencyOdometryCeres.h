// Drop-in for the reference's phovo/include/CPhotoconsistencyOdometryCeres.h: the same namespace, class name, template
// parameters and public methods, forwarding to the MI355X library through the C ABI of phovo_hip.h
// (PHOVO_OBJECTIVE_TRUST_REGION: bilinear samples, the exact warp Jacobian and a Levenberg-Marquardt trust region per
// level, gn_trust_region_kernel.hip).  Ceres is not needed: the derivatives are hand-derived.
//
//   #include "phovo/CPhotoconsistencyOdometryCeres.h"
//   phovo::Ceres::CPhotoconsistencyOdometryCeres<unsigned char, double> odometry;
//
// The types come from the same place as CPhotoconsistencyOdometryAnalytic.h's (PHOVO_HIP_USE_REFERENCE_TYPES or
// phovo/compat/).  ReadConfigurationFile reads the config_*_ceres.yml keys (reference :526-576), and Optimize() prints one
// "Ceres Solver Report" line per optimised level to stdout, as the reference does after each solve (:494).  Extensions
// other than the reference's are refused (std::runtime_error, PHOVO_E_UNSUPPORTED), and so is the inherited
// GetPairSystem(); this objective's system is GetObjectiveSystem().
#ifndef PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_CERES_H
#define PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_CERES_H

#include <cstdio>

#include "phovo/CPhotoconsistencyOdometryAnalytic.h"

namespace phovo {
namespace Ceres {

template <class TPixel, class TCoordinate>
class CPhotoconsistencyOdometryCeres : public phovo::Analytic::CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> {
 public:
  typedef phovo::Analytic::CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> Base;
  typedef typename Base::CoordinateType CoordinateType;
  typedef typename Base::IntensityImageType IntensityImageType;
  typedef typename Base::DepthImageType DepthImageType;
  typedef typename Base::Matrix33Type Matrix33Type;
  typedef typename Base::Matrix44Type Matrix44Type;
  typedef typename Base::Vector6Type Vector6Type;
  typedef typename Base::Vector4Type Vector4Type;

  explicit CPhotoconsistencyOdometryCeres(int device = 0) : Base(device)
  {
    Base::Check(phovo_odometry_set_objective(Base::Handle(), PHOVO_OBJECTIVE_TRUST_REGION), "CPhotoconsistencyOdometryCeres()");
  }

  // Optimize() (:433-500), then the summary line Ceres's BriefReport gives for every level it solved, coarse to fine.
  void Optimize()
  {
    Base::Optimize();
    const phovo_trust_region_report rep = GetSolverReport();
    for (int level = PHOVO_MAX_LEVELS - 1; level >= 0; level--) {
      const phovo_trust_region_level &r = rep.level[level];
      if (r.termination == PHOVO_TR_SKIPPED) continue;
      std::printf("Ceres Solver Report: Iterations: %d, Initial cost: %e, Final cost: %e, Termination: %s\n", r.steps + 1,
                  r.initial_cost, r.final_cost, TerminationName(r.termination));
    }
    std::fflush(stdout);
  }

  // Not in the reference: what the solver did on each level (steps, accepted steps, termination, costs, radius, rows,
  // Jacobi scaling).
  phovo_trust_region_report GetSolverReport() const
  {
    phovo_trust_region_report r;
    Base::Check(phovo_odometry_get_trust_region_report(Base::Handle(), &r), "GetSolverReport");
    return r;
  }

  // Not in the reference: J^T J, J^T r, r^T r and the row count at the optimal state on the finest level the configuration
  // optimises -- what ceres::Covariance works from.  cost is r^T r: TWICE Ceres's cost and twice GetSolverReport()'s
  // final_cost.  Evaluated on demand; std::runtime_error (PHOVO_E_NOT_READY) before Optimize() and after a Set*Frame since.
  phovo_pair_system GetObjectiveSystem() const
  {
    phovo_pair_system s;
    Base::Check(phovo_odometry_get_objective_system(Base::Handle(), &s), "GetObjectiveSystem");
    return s;
  }

  // Not in the reference: the solver options, per level (ReadConfigurationFile sets them from the file).
  void SetTrustRegionOptions(const phovo_trust_region_options &opt)
  {
    Base::Check(phovo_odometry_set_trust_region_options(Base::Handle(), &opt), "SetTrustRegionOptions");
  }

  static const char *TerminationName(int termination)
  {
    switch (termination) {
      case PHOVO_TR_MAX_ITERATIONS: return "NO_CONVERGENCE";
      case PHOVO_TR_INVALID_STEP:
      case PHOVO_TR_EVALUATION_FAILED: return "FAILURE";
      default: return "CONVERGENCE";
    }
  }
};

}  // namespace Ceres
}  // namespace phovo
#endif
