// Device probe of rotate_system of csrc/gn_device.hpp (included unchanged): one wave per case takes caller-supplied totals of
// the twist basis -- h[21], g[6] -- and the five rotation constants (cos yaw, sin yaw, temp3, temp14, temp15) through the
// function, every lane with the same inputs as in the kernels' serial section, and every lane copies out the 27 values it
// holds afterwards.  Loaded with ctypes by tests/test_gpu_system_rotation.py; built by `make -C csrc rotation-probe` into
// csrc/build/, never into the product library.
#include "gn_device.hpp"

using namespace phovo_hip;

constexpr int PROBE_IN = 32;       // 21 + 6 totals, 5 constants
constexpr int PROBE_OUT = 27;

__global__ void __launch_bounds__(WAVE) system_rotation_probe_kernel(const double *in, double *out)
{
  const double *src = in + (size_t)blockIdx.x * PROBE_IN;
  double h[21], g[6];
#pragma unroll
  for (int q = 0; q < 21; q++) h[q] = src[q];
#pragma unroll
  for (int i = 0; i < 6; i++) g[i] = src[21 + i];
  rotate_system(h, g, src[27], src[28], src[29], src[30], src[31]);
  double *o = out + ((size_t)blockIdx.x * WAVE + threadIdx.x) * PROBE_OUT;
#pragma unroll
  for (int q = 0; q < 21; q++) o[q] = h[q];
#pragma unroll
  for (int i = 0; i < 6; i++) o[21 + i] = g[i];
}

extern "C" int system_rotation_probe_inputs() { return PROBE_IN; }
extern "C" int system_rotation_probe_outputs() { return PROBE_OUT; }
extern "C" int system_rotation_probe_lanes() { return WAVE; }

// in: n_cases x 32 doubles (h[21], g[6], cos yaw, sin yaw, temp3, temp14, temp15); out: n_cases x 64 lanes x 27 doubles.
// Returns a hipError_t (0 = success).
extern "C" int system_rotation_probe_run(const double *in, int n_cases, double *out)
{
  if (n_cases <= 0) return (int)hipErrorInvalidValue;
  const size_t in_bytes = sizeof(double) * PROBE_IN * (size_t)n_cases;
  const size_t out_bytes = sizeof(double) * PROBE_OUT * WAVE * (size_t)n_cases;
  double *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(system_rotation_probe_kernel, dim3(n_cases), dim3(WAVE), 0, 0, d_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}
