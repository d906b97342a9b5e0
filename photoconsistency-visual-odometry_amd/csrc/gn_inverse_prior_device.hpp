// The Gaussian pose prior of the inverse-compositional aligners (gn_inverse_prior_kernel.hip): the logarithm
// on SE(3) and wave 0's serial section with the prior's two additions in front of the solve.  Everything is
// __forceinline__ in an anonymous namespace, as in gn_inverse_device.hpp, whose se3_exp and euler_from_rotation_lane0 it uses.
#pragma once

#include <hip/hip_runtime.h>

#include "gn_inverse_device.hpp"

namespace phovo_hip {

namespace {

// e = Log(R, t), a twist (nu, omega), the inverse of se3_exp:
//   w = vee(R - R^T) / 2, s = |w|, c = (tr R - 1) / 2, th = atan2(s, c), omega = (th / s) w,
//   nu = (I - W / 2 + D W^2) t,  W = [omega]x,  D = (1 - (th / 2) cot(th / 2)) / th^2;
// below th^2 = 1e-8 the two factors come from their series through th^4 (th / s = 1 + th^2 / 6 + 7 th^4 / 360,
// D = 1 / 12 + th^2 / 720 + th^4 / 30240).  The whole wave calls this with a wave-uniform (R, t); sin and cos of th / 2 are
// pose_sincos_lane0's.  Finite wherever s != 0 (a rotation by exactly pi has s = 0: outside the contract, as everything
// beyond 3.0 rad).
__device__ __forceinline__ void se3_log(const double (&R)[9], const double (&t)[3], int lane, double (&e)[6])
{
  const double wx = 0.5 * (R[7] - R[5]), wy = 0.5 * (R[2] - R[6]), wz = 0.5 * (R[3] - R[1]);
  const double s = sqrt(wx * wx + wy * wy + wz * wz);
  const double c = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
  const double th = atan2(s, c);
  const double th2 = th * th;
  double k, D;
  if (th2 < 1e-8) {
    k = 1.0 + th2 * (1.0 / 6.0 + th2 * (7.0 / 360.0));
    D = 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0));
  } else {
    const double hf = 0.5 * th;
    double sh, ch, s1, c1, s2, c2;
    pose_sincos_lane0(hf, hf, hf, lane, sh, ch, s1, c1, s2, c2);
    sh = uniform_f64(sh);                  // lane 0's, to every lane: everything below stays wave-uniform
    ch = uniform_f64(ch);
    k = th / s;
    D = (1.0 - hf * ch / sh) / th2;
  }
  const double ox = k * wx, oy = k * wy, oz = k * wz;
  const double ax = oy * t[2] - oz * t[1], ay = oz * t[0] - ox * t[2], az = ox * t[1] - oy * t[0];       // W t
  const double bx = oy * az - oz * ay, by = oz * ax - ox * az, bz = ox * ay - oy * ax;                   // W^2 t
  e[0] = (t[0] - 0.5 * ax) + D * bx;
  e[1] = (t[1] - 0.5 * ay) + D * by;
  e[2] = (t[2] - 0.5 * az) + D * bz;
  e[3] = ox; e[4] = oy; e[5] = oz;
}

// A pair's prior block as the engine lays it out (doubles): R_p row-major, t_p, the upper triangle of Lambda in
// solve6_ldlt's order, and 1.0 where Lambda has a non-zero entry, else 0.0.  The kernel keeps it in LDS with the pair's
// record behind it: e[6] and e^T Lambda e at the pose the level ended on.
enum { PRIOR_RP = 0, PRIOR_TP = 9, PRIOR_LAMBDA = 12, PRIOR_ACTIVE = 33, PRIOR_DOUBLES = 34, PRIOR_OUT = 34, PRIOR_LDS_DOUBLES = 42 };

// e = Log(T_p^-1 T) = Log(R_p^T R, R_p^T (t - t_p)); pr is the block in LDS.
__device__ __forceinline__ void prior_error(const double *pr, const double (&R)[9], const double (&t)[3], int lane,
                                            double (&e)[6])
{
  double Rp[9], d[3], Rr[9], tr[3];
#pragma unroll
  for (int i = 0; i < 9; i++) Rp[i] = pr[PRIOR_RP + i];
#pragma unroll
  for (int i = 0; i < 3; i++) d[i] = t[i] - pr[PRIOR_TP + i];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) Rr[3 * i + j] = Rp[i] * R[j] + Rp[3 + i] * R[3 + j] + Rp[6 + i] * R[6 + j];
    tr[i] = Rp[i] * d[0] + Rp[3 + i] * d[1] + Rp[6 + i] * d[2];
  }
  se3_log(Rr, tr, lane, e);
}

// Lambda e from the block's upper triangle (read here, so that no copy of Lambda stays live across the solve).
__device__ __forceinline__ void prior_lambda_times(const double *pr, const double (&e)[6], double (&le)[6])
{
  double lam[21];
#pragma unroll
  for (int i = 0; i < 21; i++) lam[i] = pr[PRIOR_LAMBDA + i];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) v += lam[i <= j ? tri(i, j) : tri(j, i)] * e[j];
    le[i] = v;
  }
}

// inverse_solve_compose with the prior: between the fixed-order sum and the solve,
//   e = Log(T_p^-1 T),  H' = H + s_L Lambda,  g' = g + s_L Lambda e,
// then xi = -lambda H'^-1 g' composed as there; termination and the reported norm take ||g'||.  With Lambda = 0 or s_L = 0
// wave 0 takes inverse_solve_compose ITSELF (one wave-uniform branch around the whole section, so that the compiler meets
// that function's basic blocks as it meets them in the kernels without a prior: every bit is theirs -- also where e is
// not finite).  When the level ends, lane 0 leaves e and e^T Lambda e at the new pose in the record behind the block.
__device__ __forceinline__ void prior_record(int lane, double *pr, const double (&Rn)[9], const double (&tn)[3], bool has_lambda)
{
  double e[6], le[6];
  prior_error(pr, Rn, tn, lane, e);
  prior_lambda_times(pr, e, le);
  double cost = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) cost += e[i] * le[i];
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; i++) pr[PRIOR_OUT + i] = e[i];
    pr[PRIOR_OUT + 6] = has_lambda ? cost : 0.0;
  }
}

template <int NROWS>
__device__ __forceinline__ void inverse_prior_solve_compose(int lane, const PairLds L, double *pr, double level_scale,
                                                            double lambda, int max_iter, double min_grad_norm, int iteration,
                                                            double &last_gnorm, int &last_valid)
{
  const bool has_lambda = pr[PRIOR_ACTIVE] != 0.0;
  if (!(has_lambda && level_scale != 0.0)) {                              // (wave-uniform)
    inverse_solve_compose<NROWS>(lane, L, lambda, max_iter, min_grad_norm, iteration, last_gnorm, last_valid);
    if (__builtin_amdgcn_readfirstlane(L.ctl[CTL_DONE])) {                // (lane 0's stores of this wave, read back by the wave)
      double Rn[9], tn[3];
      rt_constants_read(L.cst, Rn, tn);
      prior_record(lane, pr, Rn, tn, has_lambda);
    }
    return;
  }
  double h[21], g[6];
  sum_rows_broadcast<NROWS>(lane, L.red, h, g, last_valid);
  double R[9], t[3];
  rt_constants_read(L.cst, R, t);
  {
    double e[6], le[6];
    prior_error(pr, R, t, lane, e);
    prior_lambda_times(pr, e, le);
#pragma unroll
    for (int i = 0; i < 21; i++) h[i] += level_scale * pr[PRIOR_LAMBDA + i];
#pragma unroll
    for (int i = 0; i < 6; i++) g[i] += level_scale * le[i];
  }
  double step[6], xi[6];
  solve6_ldlt(h, g, step);
#pragma unroll
  for (int i = 0; i < 6; i++) xi[i] = -lambda * step[i];
  double ER[9], Et[3], Rn[9], tn[3];
  se3_exp(xi, lane, ER, Et);
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
    prior_record(lane, pr, Rn, tn, has_lambda);
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
