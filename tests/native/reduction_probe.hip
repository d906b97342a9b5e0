// Device probe of the sums reduction of csrc/gn_device.hpp (included unchanged): one workgroup of 1, 4, 8 or 16 waves per
// case takes caller-supplied per-lane accumulators -- NRED doubles per lane -- through exactly what the level kernels run
// behind pass 2: the wave butterfly and its row store (reduce_wave_to_row), the barrier, and wave 0's fixed-order
// cross-wave sum and broadcast (sum_rows_broadcast).  Lanes 0 and 63 of wave 0 copy out the 28 totals they were handed
// (h[21], g[6] and the raw total of the row-count slot) and the row count as the kernels read it.  Loaded with ctypes by
// tests/test_gpu_reduction_order.py; built by `make -C csrc reduction-probe` into csrc/build/, never into the product library.
#include "gn_device.hpp"

using namespace phovo_hip;

constexpr int PROBE_TOTALS = 28;

template <int NW>
__global__ void __launch_bounds__(NW * WAVE) reduction_probe_kernel(const double *in, double *out, int *n_valid_out)
{
  __shared__ double s_red[NW * NRED];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const double *src = in + ((size_t)blockIdx.x * (NW * WAVE) + (size_t)tid) * NRED;
  double acc[NRED];
#pragma unroll
  for (int j = 0; j < NRED; j++) acc[j] = src[j];
  reduce_wave_to_row(acc, lane, wave, s_red);
  __syncthreads();
  if (wave == 0) {
    double h[21], g[6];
    int n_valid;
    sum_rows_broadcast<NW>(lane, s_red, h, g, n_valid);
    if (lane == 0 || lane == WAVE - 1) {
      const size_t slot = (size_t)blockIdx.x * 2 + (lane == 0 ? 0 : 1);
      double *o = out + slot * PROBE_TOTALS;
#pragma unroll
      for (int q = 0; q < 21; q++) o[q] = h[q];
#pragma unroll
      for (int i = 0; i < 6; i++) o[21 + i] = g[i];
      o[RED_VALID] = s_red[RED_VALID];
      n_valid_out[slot] = n_valid;
    }
  }
}

extern "C" int reduction_probe_values_per_lane() { return NRED; }
extern "C" int reduction_probe_totals() { return PROBE_TOTALS; }

// in: n_cases x (waves * 64) lanes x NRED doubles; out: n_cases x 2 (lane 0, lane 63) x 28 doubles; n_valid: n_cases x 2.
// waves: 1, 4, 8 or 16.  Returns a hipError_t (0 = success).
extern "C" int reduction_probe_run(const double *in, int n_cases, int waves, double *out, int *n_valid)
{
  if (n_cases <= 0 || (waves != 1 && waves != 4 && waves != 8 && waves != 16)) return (int)hipErrorInvalidValue;
  const size_t in_bytes = sizeof(double) * NRED * WAVE * (size_t)waves * (size_t)n_cases;
  const size_t out_bytes = sizeof(double) * PROBE_TOTALS * 2 * (size_t)n_cases;
  const size_t nv_bytes = sizeof(int) * 2 * (size_t)n_cases;
  double *d_in = nullptr, *d_out = nullptr;
  int *d_nv = nullptr;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_nv, nv_bytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid(n_cases), block(waves * WAVE);
    if (waves == 1) hipLaunchKernelGGL(reduction_probe_kernel<1>, grid, block, 0, 0, d_in, d_out, d_nv);
    else if (waves == 4) hipLaunchKernelGGL(reduction_probe_kernel<4>, grid, block, 0, 0, d_in, d_out, d_nv);
    else if (waves == 8) hipLaunchKernelGGL(reduction_probe_kernel<8>, grid, block, 0, 0, d_in, d_out, d_nv);
    else hipLaunchKernelGGL(reduction_probe_kernel<16>, grid, block, 0, 0, d_in, d_out, d_nv);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(n_valid, d_nv, nv_bytes, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (d_nv) (void)hipFree(d_nv);
  return (int)e;
}
