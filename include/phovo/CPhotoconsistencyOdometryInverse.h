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
// GetPairSystem() and GetSampledSystem(): this objective's twist-basis system has no call yet.
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
};

}  // namespace Analytic
}  // namespace phovo
#endif
