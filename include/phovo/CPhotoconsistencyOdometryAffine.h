// Not in the reference: the photometric aligner with a per-pair gain and offset estimated jointly with the pose, with the
// class shape of CPhotoconsistencyOdometryAnalytic, forwarding to the MI355X library through the C ABI of phovo_hip.h
// (PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE: bilinear samples, the exact warp Jacobian, the residual
// I1 - (1 + alpha) I0 - beta and an 8 x 8 Gauss-Newton system per iteration, gn_affine_kernel.hip).
//
//   #include "phovo/CPhotoconsistencyOdometryAffine.h"
//   phovo::Analytic::CPhotoconsistencyOdometryAffine<unsigned char, double> odometry;
//
// The types come from the same place as CPhotoconsistencyOdometryAnalytic.h's (PHOVO_HIP_USE_REFERENCE_TYPES or
// phovo/compat/).  ReadConfigurationFile reads the config_*_analytic.yml keys.  Extensions are refused
// (std::runtime_error, PHOVO_E_UNSUPPORTED), and so is the inherited GetPairSystem(); the inherited GetSampledSystem()
// returns the 8 x 8 system (pose, alpha, beta) at the optimum, at the (alpha, beta) of the last Optimize().
#ifndef PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_AFFINE_H
#define PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_AFFINE_H

#include "phovo/CPhotoconsistencyOdometryAnalytic.h"

namespace phovo {
namespace Analytic {

template <class TPixel, class TCoordinate>
class CPhotoconsistencyOdometryAffine : public CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> {
 public:
  typedef CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> Base;
  typedef typename Base::CoordinateType CoordinateType;
  typedef typename Base::IntensityImageType IntensityImageType;
  typedef typename Base::DepthImageType DepthImageType;
  typedef typename Base::Matrix33Type Matrix33Type;
  typedef typename Base::Matrix44Type Matrix44Type;
  typedef typename Base::Vector6Type Vector6Type;
  typedef typename Base::Vector4Type Vector4Type;

  explicit CPhotoconsistencyOdometryAffine(int device = 0) : Base(device)
  {
    Base::Check(phovo_odometry_set_objective(Base::Handle(), PHOVO_OBJECTIVE_PHOTOMETRIC_AFFINE), "CPhotoconsistencyOdometryAffine()");
  }

  // (alpha, beta) of the last Optimize(): the target's intensities are modelled as (1 + alpha) I0 + beta.
  void GetIllumination(double &alpha, double &beta) const
  {
    double ab[2];
    Base::Check(phovo_odometry_get_illumination(Base::Handle(), ab), "GetIllumination");
    alpha = ab[0];
    beta = ab[1];
  }
};

}  // namespace Analytic
}  // namespace phovo
#endif
