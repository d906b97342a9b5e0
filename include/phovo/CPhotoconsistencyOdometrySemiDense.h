// Not in the reference: the inverse-compositional aligner of CPhotoconsistencyOdometryInverse on the source pixels selected
// once per level by depth and gradient magnitude, with the class shape of CPhotoconsistencyOdometryAnalytic, forwarding to the
// MI355X library through the C ABI of phovo_hip.h (PHOVO_OBJECTIVE_INVERSE_SEMIDENSE: pixel k is selected iff its depth is
// valid and GX0_k^2 + GY0_k^2 >= tau_L^2; gn_inverse_semidense_kernel.hip).
//
//   #include "phovo/CPhotoconsistencyOdometrySemiDense.h"
//   phovo::Analytic::CPhotoconsistencyOdometrySemiDense<unsigned char, double> odometry;
//
// The types come from the same place as CPhotoconsistencyOdometryAnalytic.h's (PHOVO_HIP_USE_REFERENCE_TYPES or
// phovo/compat/).  ReadConfigurationFile reads the config_*_analytic.yml keys and the optional key
// `min_pixel_gradient (at each level)`.  SetSourceFrame also builds the source's gradient planes.  Extensions are refused
// (std::runtime_error, PHOVO_E_UNSUPPORTED), and so is every Get...System().
#ifndef PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_SEMIDENSE_H
#define PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_SEMIDENSE_H

#include "phovo/CPhotoconsistencyOdometryAnalytic.h"

namespace phovo {
namespace Analytic {

template <class TPixel, class TCoordinate>
class CPhotoconsistencyOdometrySemiDense : public CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> {
 public:
  typedef CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> Base;
  typedef typename Base::CoordinateType CoordinateType;
  typedef typename Base::IntensityImageType IntensityImageType;
  typedef typename Base::DepthImageType DepthImageType;
  typedef typename Base::Matrix33Type Matrix33Type;
  typedef typename Base::Matrix44Type Matrix44Type;
  typedef typename Base::Vector6Type Vector6Type;
  typedef typename Base::Vector4Type Vector4Type;

  explicit CPhotoconsistencyOdometrySemiDense(int device = 0) : Base(device)
  {
    Base::Check(phovo_odometry_set_objective(Base::Handle(), PHOVO_OBJECTIVE_INVERSE_SEMIDENSE),
                "CPhotoconsistencyOdometrySemiDense()");
  }

  // tau_L per level (phovo_semidense_options; the default, 0 everywhere, selects every depth-valid pixel).
  void SetSemiDenseOptions(const phovo_semidense_options &opt)
  {
    Base::Check(phovo_odometry_set_semidense_options(Base::Handle(), &opt), "SetSemiDenseOptions");
  }
  phovo_semidense_options GetSemiDenseOptions() const
  {
    phovo_semidense_options opt;
    Base::Check(phovo_odometry_get_semidense_options(Base::Handle(), &opt), "GetSemiDenseOptions");
    return opt;
  }
  // Per level, the selected pixels of the last Optimize().
  phovo_semidense_report GetSemiDenseReport() const
  {
    phovo_semidense_report r;
    Base::Check(phovo_odometry_get_semidense_report(Base::Handle(), &r), "GetSemiDenseReport");
    return r;
  }
};

}  // namespace Analytic
}  // namespace phovo
#endif
