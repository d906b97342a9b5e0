// Not in the reference: the photometric residual aligned inverse-compositionally (Baker & Matthews), with the class shape of
// CPhotoconsistencyOdometryAnalytic, forwarding to the MI355X library through the C ABI of phovo_hip.h
// (PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL: bilinear samples of the target, the Jacobian (a, p x a) from the source frame's own
// gradient, the twist step composed on SE(3), gn_inverse_kernel.hip).
//
//   #include "phovo/CPhotoconsistencyOdometryInverse.h"
//   phovo::Analytic::CPhotoconsistencyOdometryInverse<unsigned char, double> odometry;
//
// The types come from the same place as CPhotoconsistencyOdometryAnalytic.h's (PHOVO_HIP_USE_REFERENCE_TYPES or
// phovo/compat/).  ReadConfigurationFile reads the config_*_analytic.yml keys.  SetSourceFrame also builds the source's
// gradient planes.  Extensions are refused (std::runtime_error, PHOVO_E_UNSUPPORTED), and so are the inherited
// GetPairSystem() and GetSampledSystem(), which speak the Euler basis; this objective's system is GetInverseSystem(), in
// the twist basis.
#ifndef PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_INVERSE_H
#define PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_INVERSE_H

#include "phovo/CPhotoconsistencyOdometryAnalytic.h"

namespace phovo {
namespace Analytic {

template <class TPixel, class TCoordinate>
class CPhotoconsistencyOdometryInverse : public CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> {
 public:
  typedef CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> Base;
  typedef typename Base::CoordinateType CoordinateType;
  typedef typename Base::IntensityImageType IntensityImageType;
  typedef typename Base::DepthImageType DepthImageType;
  typedef typename Base::Matrix33Type Matrix33Type;
  typedef typename Base::Matrix44Type Matrix44Type;
  typedef typename Base::Vector6Type Vector6Type;
  typedef typename Base::Vector4Type Vector4Type;

  explicit CPhotoconsistencyOdometryInverse(int device = 0) : Base(device)
  {
    Base::Check(phovo_odometry_set_objective(Base::Handle(), PHOVO_OBJECTIVE_INVERSE_COMPOSITIONAL), "CPhotoconsistencyOdometryInverse()");
  }

  // sum J J^T, sum J r, sum r^2 and the row count at the optimal state on the finest level the configuration optimises, in
  // the twist basis (nu, omega) of the right-hand perturbation T Exp(xi): xi lives in the SOURCE camera's frame, and
  // information^-1 * cost / (rows - 6) is its covariance (a caller who perturbs on the left applies Ad_T).  Evaluated on
  // demand; std::runtime_error (PHOVO_E_NOT_READY) before Optimize() and after a Set*Frame since.
  phovo_pair_system GetInverseSystem() const
  {
    phovo_pair_system s;
    Base::Check(phovo_odometry_get_inverse_system(Base::Handle(), &s), "GetInverseSystem");
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
