// Drop-in for the reference's phovo/include/CPhotoconsistencyOdometryBiObjective.h: the same namespace, class name,
// template parameters and public methods, forwarding to the MI355X library through the C ABI of phovo_hip.h
// (PHOVO_OBJECTIVE_BIOBJECTIVE: photometric and depth error together, gn_biobjective_kernel.hip).
//
//   #include "phovo/CPhotoconsistencyOdometryBiObjective.h"
//   phovo::Analytic::CPhotoconsistencyOdometryBiObjective<unsigned char, double> odometry;
//
// The types come from the same place as CPhotoconsistencyOdometryAnalytic.h's (PHOVO_HIP_USE_REFERENCE_TYPES or
// phovo/compat/).  It differs from that class in one method only: SetTargetFrame keeps the target's depth (reference
// :566-578), so the depth image must be valid.  Plane storage, sampling and Huber extensions other than the reference's
// are refused (std::runtime_error, PHOVO_E_UNSUPPORTED), and so is the inherited GetPairSystem(); this objective's system
// is GetObjectiveSystem().
#ifndef PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_BIOBJECTIVE_H
#define PHOVO_HIP_CPHOTOCONSISTENCY_ODOMETRY_BIOBJECTIVE_H

#include "phovo/CPhotoconsistencyOdometryAnalytic.h"

namespace phovo {
namespace Analytic {

template <class TPixel, class TCoordinate>
class CPhotoconsistencyOdometryBiObjective : public CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> {
 public:
  typedef CPhotoconsistencyOdometryAnalytic<TPixel, TCoordinate> Base;
  typedef typename Base::CoordinateType CoordinateType;
  typedef typename Base::IntensityImageType IntensityImageType;
  typedef typename Base::DepthImageType DepthImageType;
  typedef typename Base::Matrix33Type Matrix33Type;
  typedef typename Base::Matrix44Type Matrix44Type;
  typedef typename Base::Vector6Type Vector6Type;
  typedef typename Base::Vector4Type Vector4Type;

  explicit CPhotoconsistencyOdometryBiObjective(int device = 0) : Base(device)
  {
    Base::Check(phovo_odometry_set_objective(Base::Handle(), PHOVO_OBJECTIVE_BIOBJECTIVE), "CPhotoconsistencyOdometryBiObjective()");
  }

  // The target keeps its depth: the depth pyramid, its gradients and the depth gain are built from it (reference :573-577).
  void SetTargetFrame(const IntensityImageType &intensityImage, const DepthImageType &depthImage)
  {
    if (intensityImage.rows != depthImage.rows || intensityImage.cols != depthImage.cols)
      throw std::runtime_error("SetTargetFrame: intensity and depth sizes differ");
    Base::Check(phovo_odometry_set_target_frame(Base::Handle(), intensityImage.data, static_cast<size_t>(intensityImage.step),
                                                reinterpret_cast<const double *>(depthImage.data),
                                                static_cast<size_t>(depthImage.step), intensityImage.cols,
                                                intensityImage.rows), "SetTargetFrame");
  }

  // Not in the reference: J^T J and J^T r of the 2N-row system, r^T r over all 2N residuals and the contributing pixels at
  // the optimal state on the finest level the configuration optimises.  Evaluated on demand; std::runtime_error
  // (PHOVO_E_NOT_READY) before Optimize() and after a Set*Frame since.
  phovo_pair_system GetObjectiveSystem() const
  {
    phovo_pair_system s;
    Base::Check(phovo_odometry_get_objective_system(Base::Handle(), &s), "GetObjectiveSystem");
    return s;
  }
};

}  // namespace Analytic
}  // namespace phovo
#endif
