// What the inverse-compositional aligners share behind their pixel loops (gn_inverse_kernel.hip and
// gn_inverse_robust_kernel.hip): the exponential on SE(3), the Euler angles of a rotation matrix, and wave 0's serial
// section -- fixed-order sum, 6 x 6 solve, twist, composition onto (R, t), termination, the state at the level's exit
// (DESIGN.md §20 items 4-7).  Everything is __forceinline__ in an anonymous namespace, as in gn_sampled_device.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "gn_sampled_device.hpp"

namespace phovo_hip {

namespace {

// (E_R, E_t) = Exp(xi), xi = (nu, omega): E_R = I + A W + B W^2 (Rodrigues), E_t = (I + B W + C W^2) nu with W = [omega]x,
// A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3 = (1 - A) / th^2; below th^2 = 1e-8 the three come
// from their Taylor series through th^4 (the next term is below 1e-26 relative).  The whole wave calls this with a
// wave-uniform xi (the sines are pose_sincos_lane0's: its hand-written polynomials up to pi / 4, the device library's beyond).
__device__ __forceinline__ void se3_exp(const double (&xi)[6], int lane, double (&ER)[9], double (&Et)[3])
{
  const double wx = xi[3], wy = xi[4], wz = xi[5];
  const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
  const double th2 = xx + yy + zz;
  double A, B, C;
  if (th2 < 1e-8) {
    A = 1.0 - th2 * (1.0 / 6.0 - th2 * (1.0 / 120.0));
    B = 0.5 - th2 * (1.0 / 24.0 - th2 * (1.0 / 720.0));
    C = 1.0 / 6.0 - th2 * (1.0 / 120.0 - th2 * (1.0 / 5040.0));
  } else {
    const double th = sqrt(th2);
    double sn, cs, sh, ch, s2, c2;
    pose_sincos_lane0(th, 0.5 * th, th, lane, sn, cs, sh, ch, s2, c2);    // lane 1 worked on th / 2: lane 0 has both sines
    sn = uniform_f64(sn);                  // lane 0's, to every lane: everything below stays wave-uniform
    sh = uniform_f64(sh);
    A = sn / th;
    B = 2.0 * sh * sh / th2;               // 1 - cos th = 2 sin^2(th / 2): no cancellation (E_t has B W nu, first order in th)
    C = (1.0 - A) / th2;
  }
  const double xy = wx * wy, xz = wx * wz, yz = wy * wz;
  auto fill = [&](double (&M)[9], double a, double b) {                   // I + a W + b W^2,  W^2 = omega omega^T - th^2 I
    M[0] = 1.0 - b * (yy + zz); M[1] = b * xy - a * wz;     M[2] = b * xz + a * wy;
    M[3] = b * xy + a * wz;     M[4] = 1.0 - b * (xx + zz); M[5] = b * yz - a * wx;
    M[6] = b * xz - a * wy;     M[7] = b * yz + a * wx;     M[8] = 1.0 - b * (xx + yy);
  };
  fill(ER, A, B);
  double V[9];
  fill(V, B, C);
#pragma unroll
  for (int i = 0; i < 3; i++) Et[i] = V[3 * i] * xi[0] + V[3 * i + 1] * xi[1] + V[3 * i + 2] * xi[2];
}

// (yaw, pitch, roll) of a rotation matrix, the inverse of eigenPose: yaw = atan2(R10, R00), pitch = atan2(-R20,
// sqrt(R00^2 + R10^2)), roll = atan2(R21, R22).  Lanes 0, 1, 2 take one angle each (ONE atan2 issue); valid in lane 0.
__device__ __forceinline__ void euler_from_rotation_lane0(const double (&R)[9], int lane, double &yaw, double &pitch, double &roll)
{
  const double num = lane == 1 ? -R[6] : (lane == 2 ? R[7] : R[3]);
  const double den = lane == 1 ? sqrt(R[0] * R[0] + R[3] * R[3]) : (lane == 2 ? R[8] : R[0]);
  const double ang = atan2(num, den);
  yaw = ang;
  pitch = dpp_f64<DPP_QUAD_BCAST1>(ang);
  roll = dpp_f64<DPP_QUAD_BCAST2>(ang);
}

// Called by wave 0 behind the barrier that follows reduce_wave_to_row: the fixed-order sum of the NROWS rows, the 6 x 6
// solve, the twist, its exponential composed onto (R, t) in the constant block, termination (update_and_terminate's rule,
// with the finite test on (R, t)) and, when the level ends, the state read off (R, t).
template <int NROWS>
__device__ __forceinline__ void inverse_solve_compose(int lane, const PairLds L, double lambda, int max_iter,
                                                      double min_grad_norm, int iteration, double &last_gnorm, int &last_valid)
{
  double h[21], g[6];
  sum_rows_broadcast<NROWS>(lane, L.red, h, g, last_valid);
  double step[6], xi[6];
  solve6_ldlt(h, g, step);
#pragma unroll
  for (int i = 0; i < 6; i++) xi[i] = -lambda * step[i];
  double ER[9], Et[3], R[9], t[3], Rn[9], tn[3];
  se3_exp(xi, lane, ER, Et);
  rt_constants_read(L.cst, R, t);
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      Rn[3 * i + j] = R[3 * i] * ER[j] + R[3 * i + 1] * ER[3 + j] + R[3 * i + 2] * ER[6 + j];
      finite = finite && finite_f64(Rn[3 * i + j]);
    }
    tn[i] = (R[3 * i] * Et[0] + R[3 * i + 1] * Et[1] + R[3 * i + 2] * Et[2]) + t[i];
    finite = finite && finite_f64(tn[i]);
  }
  double gn2 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) gn2 += g[i] * g[i];
  const double gnorm = sqrt(gn2);
  bool done = false;
  if (iteration + 1 >= max_iter) done = true;
  else if (gnorm < min_grad_norm) done = true;
  if (!finite) done = true;
  if (done) {                                                             // (wave-uniform)
    double yaw, pitch, roll;
    euler_from_rotation_lane0(Rn, lane, yaw, pitch, roll);
    if (lane == 0) {
      const double nan = __hiloint2double(0x7ff80000, 0);
      L.state[0] = finite ? tn[0] : nan; L.state[1] = finite ? tn[1] : nan; L.state[2] = finite ? tn[2] : nan;
      L.state[3] = finite ? yaw : nan; L.state[4] = finite ? pitch : nan; L.state[5] = finite ? roll : nan;
    }
  }
  if (lane == 0) {
    rt_constants_write(L.cst, Rn, tn);
    L.ctl[CTL_DONE] = done ? 1 : 0;
    if (!finite) L.ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_NONFINITE;
    if (last_valid < 6) L.ctl[CTL_FLAGS] |= (int)PHOVO_PAIR_RANK_DEFICIENT;
  }
  last_gnorm = gnorm;
}

}  // namespace

}  // namespace phovo_hip
