// Device probe of the arithmetic helpers of csrc/gn_device.hpp (included unchanged): fast_rcp<1|2>, round_half_up_from,
// rowcol_from_index / _floor, rowcol_advance, mad24_uniform_b, plane_load<double|float|__half> through plane_rsrc and
// frame_rsrc, solve6_ldlt, solve6_cholesky, solve8_ldlt.  One entry point per family: plain arrays in and out, one thread
// per element, 64-thread workgroups; every entry point returns a hipError_t (0 = success) and checks every HIP call.
// Loaded with ctypes by tests/test_gpu_device_arith.py; built by `make -C csrc arith-probe` into csrc/build/, never into
// the product library.
//
// The load entry point cannot leave its allocation whatever the hardware's range check includes: the caller's bytes sit
// between two guards of ARITH_PROBE_GUARD bytes of sentinel, the descriptor's base is the first payload byte, and the host
// refuses (hipErrorInvalidValue) every index whose byte address soff + idx * size, taken WITHOUT any range check, would
// fall outside guard + payload + guard.
#include <vector>

#include "gn_device.hpp"

using namespace phovo_hip;

namespace {

constexpr int GROUP = 64;
constexpr size_t ARITH_PROBE_GUARD = 64 * 1024;
constexpr unsigned char ARITH_PROBE_SENTINEL = 0xA5;

__global__ void __launch_bounds__(GROUP) rcp_kernel(const double *x, int n, int steps, double *r)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n) return;
  r[i] = steps == 1 ? fast_rcp<1>(x[i]) : fast_rcp<2>(x[i]);
}

__global__ void __launch_bounds__(GROUP) round_half_kernel(const double *v, int n, double *out)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n) return;
  out[i] = round_half_up_from(v[i]);
}

// the width is one per workgroup (make_rowcol_from_index moves 1 / W to scalar registers: it must be wave-uniform)
__global__ void __launch_bounds__(GROUP) rowcol_kernel(const int *k, const int *w_group, int floor_flag, double *c, double *r)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  const int W = __builtin_amdgcn_readfirstlane(w_group[blockIdx.x]);
  const RowColFromIndex m = make_rowcol_from_index(W);
  double cd, rd;
  if (floor_flag) rowcol_from_index_floor((double)k[i], m, cd, rd);
  else rowcol_from_index((double)k[i], m, cd, rd);
  c[i] = cd;
  r[i] = rd;
}

// one thread per walk: (row, column) of `start` by integer division, then `steps` calls of rowcol_advance, each recorded
__global__ void __launch_bounds__(GROUP) rowcol_walk_kernel(int n_walks, const int *W, const int *start, const int *step_r,
                                                            const int *step_c, const int *steps, const long long *out_off,
                                                            double *c, double *r)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n_walks) return;
  const RowColStep s = make_rowcol_step(step_r[i], step_c[i], W[i]);
  double cd = (double)(start[i] % W[i]), rd = (double)(start[i] / W[i]);
  double *co = c + out_off[i], *ro = r + out_off[i];
  for (int t = 0; t < steps[i]; t++) {
    rowcol_advance(cd, rd, s);
    co[t] = cd;
    ro[t] = rd;
  }
}

__global__ void __launch_bounds__(GROUP) mad24_kernel(const int *a, int b, const int *c, int n, int *out)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n) return;
  out[i] = mad24_uniform_b(a[i], b, c[i]);
}

template <typename T>
__global__ void __launch_bounds__(GROUP) load_kernel(const unsigned char *base, int num_records, int soff, const int *idx, int n,
                                                     double *out)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n) return;
  // soff == 0: a descriptor per plane, as the kernels build it; otherwise one per frame and the plane's offset in soff
  const __amdgpu_buffer_rsrc_t r = soff == 0 ? plane_rsrc<T>(base, num_records / (int)sizeof(T))
                                             : frame_rsrc(base, (size_t)num_records);
  out[i] = plane_load<T>(r, idx[i], soff);
}

__global__ void __launch_bounds__(GROUP) solve6_kernel(const double *h, const double *g, int n, double *x)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n) return;
  double hh[21], gg[6], xx[6];
  for (int q = 0; q < 21; q++) hh[q] = h[(size_t)i * 21 + q];
  for (int q = 0; q < 6; q++) gg[q] = g[(size_t)i * 6 + q];
  solve6_ldlt(hh, gg, xx);
  for (int q = 0; q < 6; q++) x[(size_t)i * 6 + q] = xx[q];
}

__global__ void __launch_bounds__(GROUP) solve6_chol_kernel(const double *a, const double *b, int n, double *y, int *ok)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n) return;
  double aa[21], bb[6], yy[6];
  for (int q = 0; q < 21; q++) aa[q] = a[(size_t)i * 21 + q];
  for (int q = 0; q < 6; q++) bb[q] = b[(size_t)i * 6 + q];
  const bool solved = solve6_cholesky(aa, bb, yy);
  for (int q = 0; q < 6; q++) y[(size_t)i * 6 + q] = yy[q];
  ok[i] = solved ? 1 : 0;
}

__global__ void __launch_bounds__(GROUP) solve8_kernel(const double *h, const double *g, int n, double *x)
{
  const int i = blockIdx.x * GROUP + threadIdx.x;
  if (i >= n) return;
  double hh[36], gg[NP], xx[NP];
  for (int q = 0; q < 36; q++) hh[q] = h[(size_t)i * 36 + q];
  for (int q = 0; q < NP; q++) gg[q] = g[(size_t)i * NP + q];
  solve8_ldlt(hh, gg, xx);
  for (int q = 0; q < NP; q++) x[(size_t)i * NP + q] = xx[q];
}

// Device buffers of one call: inputs uploaded on creation, everything freed on destruction; the first failing status sticks.
struct Buffers {
  hipError_t e = hipSuccess;
  std::vector<void *> owned;
  ~Buffers() { for (void *p : owned) (void)hipFree(p); }
  void *raw(size_t bytes)
  {
    void *p = nullptr;
    if (e == hipSuccess) e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess) owned.push_back(p); else p = nullptr;
    return p;
  }
  template <typename T> T *in(const T *host, size_t count)
  {
    T *p = static_cast<T *>(raw(sizeof(T) * count));
    if (e == hipSuccess && count) e = hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice);
    return p;
  }
  template <typename T> T *out(size_t count) { return static_cast<T *>(raw(sizeof(T) * count)); }
  void launched()
  {
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  template <typename T> void back(T *host, const T *dev, size_t count)
  {
    if (e == hipSuccess && count) e = hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost);
  }
};

inline dim3 groups(long long n) { return dim3((unsigned)((n + GROUP - 1) / GROUP)); }

}  // namespace

extern "C" int arith_probe_guard_bytes() { return (int)ARITH_PROBE_GUARD; }
extern "C" int arith_probe_sentinel() { return (int)ARITH_PROBE_SENTINEL; }

// r[i] = fast_rcp<steps>(x[i]), steps 1 or 2
extern "C" int arith_probe_rcp(const double *x, int n, int steps, double *r)
{
  if (n <= 0 || (steps != 1 && steps != 2)) return (int)hipErrorInvalidValue;
  Buffers b;
  const double *dx = b.in(x, n);
  double *dr = b.out<double>(n);
  if (b.e == hipSuccess) hipLaunchKernelGGL(rcp_kernel, groups(n), dim3(GROUP), 0, 0, dx, n, steps, dr);
  b.launched();
  b.back(r, dr, n);
  return (int)b.e;
}

extern "C" int arith_probe_round_half(const double *v, int n, double *out)
{
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const double *dv = b.in(v, n);
  double *d_out = b.out<double>(n);
  if (b.e == hipSuccess) hipLaunchKernelGGL(round_half_kernel, groups(n), dim3(GROUP), 0, 0, dv, n, d_out);
  b.launched();
  b.back(out, d_out, n);
  return (int)b.e;
}

// (c, r)[i] = rowcol_from_index(k[i]) (floor_flag: _floor) at width w_group[i / 64] >= 1; n is a multiple of 64
extern "C" int arith_probe_rowcol(const int *k, int n, const int *w_group, int floor_flag, double *c, double *r)
{
  if (n <= 0 || n % GROUP != 0) return (int)hipErrorInvalidValue;
  for (int q = 0; q < n / GROUP; q++) if (w_group[q] < 1) return (int)hipErrorInvalidValue;
  Buffers b;
  const int *dk = b.in(k, n), *dw = b.in(w_group, n / GROUP);
  double *dc = b.out<double>(n), *dr = b.out<double>(n);
  if (b.e == hipSuccess) hipLaunchKernelGGL(rowcol_kernel, groups(n), dim3(GROUP), 0, 0, dk, dw, floor_flag, dc, dr);
  b.launched();
  b.back(c, dc, n);
  b.back(r, dr, n);
  return (int)b.e;
}

// Walk i: from pixel start[i] of an image W[i] wide, steps[i] calls of rowcol_advance with (step_r[i], step_c[i]); the
// (column, row) after call t goes to c / r [out_off[i] + t].  total = the length of c and r.
extern "C" int arith_probe_rowcol_walk(int n_walks, const int *W, const int *start, const int *step_r, const int *step_c,
                                       const int *steps, const long long *out_off, long long total, double *c, double *r)
{
  if (n_walks <= 0 || total <= 0) return (int)hipErrorInvalidValue;
  for (int i = 0; i < n_walks; i++)
    if (W[i] < 1 || start[i] < 0 || steps[i] < 0 || out_off[i] < 0 || out_off[i] + steps[i] > total)
      return (int)hipErrorInvalidValue;
  Buffers b;
  const int *dW = b.in(W, n_walks), *ds = b.in(start, n_walks), *dsr = b.in(step_r, n_walks), *dsc = b.in(step_c, n_walks);
  const int *dn = b.in(steps, n_walks);
  const long long *doff = b.in(out_off, n_walks);
  double *dc = b.out<double>(total), *dr = b.out<double>(total);
  if (b.e == hipSuccess)
    hipLaunchKernelGGL(rowcol_walk_kernel, groups(n_walks), dim3(GROUP), 0, 0, n_walks, dW, ds, dsr, dsc, dn, doff, dc, dr);
  b.launched();
  b.back(c, dc, total);
  b.back(r, dr, total);
  return (int)b.e;
}

// out[i] = mad24_uniform_b(a[i], b, c[i]); b is a kernel argument (wave-uniform, a scalar register)
extern "C" int arith_probe_mad24(const int *a, int bval, const int *c, int n, int *out)
{
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const int *da = b.in(a, n), *dc = b.in(c, n);
  int *d_out = b.out<int>(n);
  if (b.e == hipSuccess) hipLaunchKernelGGL(mad24_kernel, groups(n), dim3(GROUP), 0, 0, da, bval, dc, n, d_out);
  b.launched();
  b.back(out, d_out, n);
  return (int)b.e;
}

// out[i] = plane_load<T>(descriptor, idx[i], soff), T by storage (0 double, 1 float, 2 __half).  The descriptor's base is the
// first of the caller's `nbytes` bytes, which sit between two sentinel guards; num_records <= nbytes bytes;
// soff == 0: plane_rsrc<T>(base, num_records / sizeof(T)), otherwise frame_rsrc(base, num_records).
extern "C" int arith_probe_load(int storage, const unsigned char *bytes, int nbytes, int num_records, int soff, const int *idx,
                                int n, double *out)
{
  const long long size = storage == 0 ? 8 : (storage == 1 ? 4 : 2);
  if (storage < 0 || storage > 2 || n <= 0 || nbytes <= 0 || num_records < 0 || num_records > nbytes || soff < 0 ||
      soff % size != 0 || num_records % size != 0)
    return (int)hipErrorInvalidValue;
  const long long guard = (long long)ARITH_PROBE_GUARD;
  for (int i = 0; i < n; i++) {
    // the address the instruction forms if nothing is range-checked: never outside the allocation.  A negative index is an
    // unsigned offset of 4 GiB less a little: admitted only where base + soff + idx * size is still inside the front guard
    // (the address then stays in the allocation even if the sum wrapped at 32 bits), which needs soff + idx * size >= -guard
    const long long at = (long long)soff + (long long)idx[i] * size;
    if (at < -guard || at + size > (long long)nbytes + guard) return (int)hipErrorInvalidValue;
  }
  const size_t total = ARITH_PROBE_GUARD + (size_t)nbytes + ARITH_PROBE_GUARD;
  Buffers b;
  unsigned char *mem = static_cast<unsigned char *>(b.raw(total));
  if (b.e == hipSuccess) b.e = hipMemset(mem, ARITH_PROBE_SENTINEL, total);
  if (b.e == hipSuccess) b.e = hipMemcpy(mem + ARITH_PROBE_GUARD, bytes, (size_t)nbytes, hipMemcpyHostToDevice);
  const int *didx = b.in(idx, n);
  double *d_out = b.out<double>(n);
  if (b.e == hipSuccess) {
    const unsigned char *base = mem + ARITH_PROBE_GUARD;
    if (storage == 0) hipLaunchKernelGGL(load_kernel<double>, groups(n), dim3(GROUP), 0, 0, base, num_records, soff, didx, n, d_out);
    else if (storage == 1) hipLaunchKernelGGL(load_kernel<float>, groups(n), dim3(GROUP), 0, 0, base, num_records, soff, didx, n, d_out);
    else hipLaunchKernelGGL(load_kernel<__half>, groups(n), dim3(GROUP), 0, 0, base, num_records, soff, didx, n, d_out);
  }
  b.launched();
  b.back(out, d_out, n);
  return (int)b.e;
}

// x[i] = solve6_ldlt(h[i], g[i]): h the upper triangle, row-major, 21 per system
extern "C" int arith_probe_solve6(const double *h, const double *g, int n, double *x)
{
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const double *dh = b.in(h, (size_t)n * 21), *dg = b.in(g, (size_t)n * 6);
  double *dx = b.out<double>((size_t)n * 6);
  if (b.e == hipSuccess) hipLaunchKernelGGL(solve6_kernel, groups(n), dim3(GROUP), 0, 0, dh, dg, n, dx);
  b.launched();
  b.back(x, dx, (size_t)n * 6);
  return (int)b.e;
}

// (y[i], ok[i]) = solve6_cholesky(a[i], b[i])
extern "C" int arith_probe_solve6_chol(const double *a, const double *rhs, int n, double *y, int *ok)
{
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const double *da = b.in(a, (size_t)n * 21), *db = b.in(rhs, (size_t)n * 6);
  double *dy = b.out<double>((size_t)n * 6);
  int *dok = b.out<int>(n);
  if (b.e == hipSuccess) hipLaunchKernelGGL(solve6_chol_kernel, groups(n), dim3(GROUP), 0, 0, da, db, n, dy, dok);
  b.launched();
  b.back(y, dy, (size_t)n * 6);
  b.back(ok, dok, n);
  return (int)b.e;
}

// x[i] = solve8_ldlt(h[i], g[i]): 36 per system
extern "C" int arith_probe_solve8(const double *h, const double *g, int n, double *x)
{
  if (n <= 0) return (int)hipErrorInvalidValue;
  Buffers b;
  const double *dh = b.in(h, (size_t)n * 36), *dg = b.in(g, (size_t)n * NP);
  double *dx = b.out<double>((size_t)n * NP);
  if (b.e == hipSuccess) hipLaunchKernelGGL(solve8_kernel, groups(n), dim3(GROUP), 0, 0, dh, dg, n, dx);
  b.launched();
  b.back(x, dx, (size_t)n * NP);
  return (int)b.e;
}
