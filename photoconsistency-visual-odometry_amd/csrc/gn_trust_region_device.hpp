// The trust-region rows' device functions, shared by the aligner (gn_trust_region_kernel.hip) and the evaluation of its
// system at given states (gn_evaluate_objective_kernels.hip): the warp of a source pixel and SampleLinear's taps.  Both
// files compile them under `#pragma clang fp contract(off)`, set BEFORE this header is included, so that the warped
// positions -- and with them the truncations and the bounds tests -- are the CPU checker's (tests/trust_region_ref.py)
// and each other's bit for bit.
#pragma once

#include "gn_device.hpp"
#include "phovo_internal.hpp"

namespace phovo_hip {

namespace {

// The warp of source pixel i (index k as a double): depth gate, back-projection, rigid motion, projection, bounds.
// Args: GNLevelArgs or GNObjectiveEvalArgs (the level view: intrinsics, depth range, size).
struct Warp {
  double px, py, pz, a0, a1, a2, q0, q1, q2, u, v;
  bool ok;
};
template <class Args>
__device__ __forceinline__ Warp warp_pixel(double kd, double d, const RowColFromIndex &rc, const Args &A,
                                           const double (&R)[9], const double (&t)[3])
{
  Warp w;
  double cd, rd;
  rowcol_from_index(kd, rc, cd, rd);
  w.pz = d;
  w.px = (cd - A.ox) * d * A.ifx;                                              // :229
  w.py = (rd - A.oy) * d * A.ify;                                              // :230
  w.a0 = R[0] * w.px + R[1] * w.py + R[2] * w.pz;                              // :234-236 (rotation part)
  w.a1 = R[3] * w.px + R[4] * w.py + R[5] * w.pz;
  w.a2 = R[6] * w.px + R[7] * w.py + R[8] * w.pz;
  w.q0 = w.a0 + t[0];
  w.q1 = w.a1 + t[1];
  w.q2 = w.a2 + t[2];
  w.u = (w.q0 * A.fx) / w.q2 + A.ox;                                           // :240 (a division)
  w.v = (w.q1 * A.fy) / w.q2 + A.oy;                                           // :241
  // :245-246 on the real values; NaN fails every comparison
  w.ok = A.min_depth < d && d < A.max_depth && w.v >= 0.0 && w.v < (double)A.h && w.u >= 0.0 && w.u < (double)A.w;
  return w;
}

// LinearInitAxis (third_party/sample.h:32-51) after SampleLinear's shift by -0.5: taps i0, i1 and the weight of i0
__device__ __forceinline__ void linear_axis(double c, int size, int &i0, int &i1, double &wgt)
{
  const double a = c - 0.5;
  const int i = (int)a;                        // truncation toward zero: a in [-0.5, 0) gives 0 and a weight above 1
  if (i > size - 2) { i0 = size - 1; i1 = size - 1; wgt = 1.0; }
  else { i0 = i; i1 = i + 1; wgt = (double)(i + 1) - a; }
}

__device__ __forceinline__ double bilinear(__amdgpu_buffer_rsrc_t r, int soff, int k11, int k12, int k21, int k22,
                                           double wx, double wy)
{
  const double p11 = plane_load<double>(r, k11, soff), p12 = plane_load<double>(r, k12, soff);
  const double p21 = plane_load<double>(r, k21, soff), p22 = plane_load<double>(r, k22, soff);
  return wy * (wx * p11 + (1.0 - wx) * p12) + (1.0 - wy) * (wx * p21 + (1.0 - wx) * p22);   // sample.h:79-80
}

}  // namespace

}  // namespace phovo_hip
