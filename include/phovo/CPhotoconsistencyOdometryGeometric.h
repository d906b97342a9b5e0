// Not in the reference: the photometric aligner with a depth row per pixel beside the intensity row, with the class shape of
// CPhotoconsistencyOdometryAnalytic, forwarding to the MI355X library through the C ABI of phovo_hip.h
// (PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC: bilinear samples of the target's intensity AND depth, the exact warp Jacobian, the
// residuals I1 - I0 and sigma (D1 - Z'), a 6 x 6 Gauss-Newton system per iteration, gn_geometric_kernel.hip).
//
//   #include "phovo/CPhotoconsistencyOdometryGeometric.h"
//   phovo::Analytic::CPhotoconsistencyOdometryGeometric<unsigned char, double> odometry;
//
// The types come from the same place as CPhotoconsistencyOdometryAnalytic.h's (PHOVO_HIP_USE_REFERENCE_TYPES or
// phovo/compat/).  SetTargetFrame USES the target's depth here.  ReadConfigurationFile reads the config_*_analytic.yml keys
// and the two optional keys "depth_weight (at each level)" and "max_depth_residual (at each level)".  Extensions are refused
// (std::runtime_error, PHOVO_E_UNSUPPORTED), and so are the inherited GetPairSystem() and GetSampledSystem(); this
// objective's system, with the photometric and the depth block apart, is GetGeometricSystem().
#ifndef PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_GEOMETRIC_H
#define PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_GEOMETRIC_H

#include "phovo/CPhotoconsistencyOdometryAnalytic.h"

namespace phovo {
namespace Analytic {

template <class TPixel, class TCoordinate>
class CPhotoconsistencyOdometryGeometric : public CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> {
 public:
  typedef CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> Base;
  typedef typename Base::CoordinateType CoordinateType;
  typedef typename Base::IntensityImageType IntensityImageType;
  typedef typename Base::DepthImageType DepthImageType;
  typedef typename Base::Matrix33Type Matrix33Type;
  typedef typename Base::Matrix44Type Matrix44Type;
  typedef typename Base::Vector6Type Vector6Type;
  typedef typename Base::Vector4Type Vector4Type;

  explicit CPhotoconsistencyOdometryGeometric(int device = 0) : Base(device)
  {
    Base::Check(phovo_odometry_set_objective(Base::Handle(), PHOVO_OBJECTIVE_PHOTOMETRIC_GEOMETRIC), "CPhotoconsistencyOdometryGeometric()");
  }

  // The depth weight and the residual gate of every level (phovo_geometric_options: settings to tune, not measured optima).
  void SetGeometricOptions(const phovo_geometric_options &opt)
  {
    Base::Check(phovo_odometry_set_geometric_options(Base::Handle(), &opt), "SetGeometricOptions");
  }
  phovo_geometric_options GetGeometricOptions() const
  {
    phovo_geometric_options opt;
    Base::Check(phovo_odometry_get_geometric_options(Base::Handle(), &opt), "GetGeometricOptions");
    return opt;
  }

  // Depth rows and the two costs of every level's last system in the last Optimize().
  phovo_geometric_report GetGeometricReport() const
  {
    phovo_geometric_report r;
    Base::Check(phovo_odometry_get_geometric_report(Base::Handle(), &r), "GetGeometricReport");
    return r;
  }

  // The Gauss-Newton system at the optimal state on the finest level the configuration optimises: the photometric and the
  // depth block apart, and their sum; evaluated on demand after Optimize().
  phovo_geometric_system GetGeometricSystem() const
  {
    phovo_geometric_system s;
    Base::Check(phovo_odometry_get_geometric_system(Base::Handle(), &s), "GetGeometricSystem");
    return s;
  }
};

}  // namespace Analytic
}  // namespace phovo
#endif
