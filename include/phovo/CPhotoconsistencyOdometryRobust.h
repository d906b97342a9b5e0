// Not in the reference: the inverse-compositional aligner of CPhotoconsistencyOdometryInverse under a Huber weight whose
// threshold follows the pair's own residuals, with the class shape of CPhotoconsistencyOdometryAnalytic, forwarding to the
// MI355X library through the C ABI of phovo_hip.h (PHOVO_OBJECTIVE_INVERSE_ROBUST: delta = scale_factor * median |r| from a
// histogram of the rows' residuals, lagging one iteration; gn_inverse_robust_kernel.hip).
//
//   #include "phovo/CPhotoconsistencyOdometryRobust.h"
//   phovo::Analytic::CPhotoconsistencyOdometryRobust<unsigned char, double> odometry;
//
// The types come from the same place as CPhotoconsistencyOdometryAnalytic.h's (PHOVO_HIP_USE_REFERENCE_TYPES or
// phovo/compat/).  ReadConfigurationFile reads the config_*_analytic.yml keys.  SetSourceFrame also builds the source's
// gradient planes.  Extensions are refused (std::runtime_error, PHOVO_E_UNSUPPORTED), and so are the inherited
// GetPairSystem() and GetSampledSystem(), which speak the Euler basis; this objective's weighted system is
// GetRobustSystem(), in the twist basis.
#ifndef PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_ROBUST_H
#define PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_ROBUST_H

#include "phovo/CPhotoconsistencyOdometryAnalytic.h"

namespace phovo {
namespace Analytic {

template <class TPixel, class TCoordinate>
class CPhotoconsistencyOdometryRobust : public CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> {
 public:
  typedef CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> Base;
  typedef typename Base::CoordinateType CoordinateType;
  typedef typename Base::IntensityImageType IntensityImageType;
  typedef typename Base::DepthImageType DepthImageType;
  typedef typename Base::Matrix33Type Matrix33Type;
  typedef typename Base::Matrix44Type Matrix44Type;
  typedef typename Base::Vector6Type Vector6Type;
  typedef typename Base::Vector4Type Vector4Type;

  explicit CPhotoconsistencyOdometryRobust(int device = 0) : Base(device)
  {
    Base::Check(phovo_odometry_set_objective(Base::Handle(), PHOVO_OBJECTIVE_INVERSE_ROBUST), "CPhotoconsistencyOdometryRobust()");
  }

  // delta = scale_factor * median |r| (phovo_robust_options; the default is 1.345 * 1.4826).
  void SetRobustOptions(const phovo_robust_options &opt)
  {
    Base::Check(phovo_odometry_set_robust_options(Base::Handle(), &opt), "SetRobustOptions");
  }
  phovo_robust_options GetRobustOptions() const
  {
    phovo_robust_options opt;
    Base::Check(phovo_odometry_get_robust_options(Base::Handle(), &opt), "GetRobustOptions");
    return opt;
  }
  // Per level, the threshold and the outlier rows of the last system of the last Optimize().
  phovo_robust_report GetRobustReport() const
  {
    phovo_robust_report r;
    Base::Check(phovo_odometry_get_robust_report(Base::Handle(), &r), "GetRobustReport");
    return r;
  }
  // The weighted system at the optimal state on the finest level the configuration optimises, with the median rule taken
  // at that state: sum w J J^T and sum w J r in the twist basis (nu, omega) of the right-hand perturbation T Exp(xi) (xi in
  // the SOURCE camera's frame), sum w r^2, the Huber and the squared cost, delta, the median, rows and outliers
  // (phovo_engine_evaluate_robust_pairs has the contract).  Evaluated on demand; std::runtime_error
  // (PHOVO_E_NOT_READY) before Optimize() and after a Set*Frame since.
  phovo_robust_system GetRobustSystem() const
  {
    phovo_robust_system s;
    Base::Check(phovo_odometry_get_robust_system(Base::Handle(), &s), "GetRobustSystem");
    return s;
  }

  // A Gaussian pose prior for every later Optimize() until ClearPosePrior() (phovo_hip.h, phovo_prior_options; DESIGN.md
  // §24): state = (x, y, z, yaw, pitch, roll) of the prior pose, information row-major 6 x 6 in the twist order (nu, omega)
  // of GetInverseSystem(), its upper triangle read.  std::runtime_error (PHOVO_E_INVALID_ARGUMENT) for a non-finite entry
  // or a negative diagonal.
  void SetPosePrior(const double state[6], const double information[36])
  {
    Base::Check(phovo_odometry_set_pose_prior(Base::Handle(), state, information), "SetPosePrior");
  }
  void ClearPosePrior() { Base::Check(phovo_odometry_clear_pose_prior(Base::Handle()), "ClearPosePrior"); }
  // The per-level scale s_L of the prior (default 1 on every level).
  void SetPriorOptions(const phovo_prior_options &opt)
  {
    Base::Check(phovo_odometry_set_prior_options(Base::Handle(), &opt), "SetPriorOptions");
  }
  phovo_prior_options GetPriorOptions() const
  {
    phovo_prior_options opt;
    Base::Check(phovo_odometry_get_prior_options(Base::Handle(), &opt), "GetPriorOptions");
    return opt;
  }
  // e = Log(T_p^-1 T) and e^T Lambda e at the optimal state of the last Optimize(), which carried a prior.
  phovo_prior_report GetPriorReport() const
  {
    phovo_prior_report r;
    Base::Check(phovo_odometry_get_prior_report(Base::Handle(), &r), "GetPriorReport");
    return r;
  }
};

}  // namespace Analytic
}  // namespace phovo
#endif
