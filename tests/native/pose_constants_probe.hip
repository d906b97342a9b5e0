// Device probe of write_pose_constants (csrc/gn_device.hpp, included unchanged): one 64-lane wave per state calls it
// exactly as the level kernels do -- wave-uniform state, every lane passing its lane index, lane 0 writing the block of
// pose constants into LDS -- and the block is copied out to global memory.  Loaded with ctypes by
// tests/test_gpu_pose_constants.py; built by `make -C csrc pose-probe` into csrc/build/, never into the product library.
#include "gn_device.hpp"

using namespace phovo_hip;

__global__ void __launch_bounds__(WAVE) pose_constants_probe_kernel(const double *states, double *out)
{
  __shared__ double s_cst[32];
  const int lane = threadIdx.x;
  const double *st = states + (size_t)blockIdx.x * 6;
  if (lane < 32) s_cst[lane] = 0.0;
  __syncthreads();
  write_pose_constants(st[0], st[1], st[2], st[3], st[4], st[5], s_cst, lane);
  __syncthreads();
  if (lane < C_COUNT) out[(size_t)blockIdx.x * C_COUNT + lane] = s_cst[lane];
}

// states: n x 6 (x, y, z, yaw, pitch, roll); out: n x pose_probe_count() doubles.  Returns a hipError_t (0 = success).
extern "C" int pose_probe_count() { return C_COUNT; }

extern "C" int pose_probe_run(const double *states, int n, double *out)
{
  if (n <= 0) return (int)hipErrorInvalidValue;
  double *d_states = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_states, sizeof(double) * 6 * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * C_COUNT * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(d_states, states, sizeof(double) * 6 * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pose_constants_probe_kernel, dim3(n), dim3(WAVE), 0, 0, d_states, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(double) * C_COUNT * (size_t)n, hipMemcpyDeviceToHost);
  if (d_states) (void)hipFree(d_states);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}
