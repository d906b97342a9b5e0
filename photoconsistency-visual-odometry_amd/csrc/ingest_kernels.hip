// Packing kernels of phovo_engine_upload_frames_device (include/phovo_hip.h): frames that already live in device memory,
// with the caller's row and frame strides, are packed into the engine's raw-frame staging buffers -- the same buffers a
// host upload fills by DMA -- so that the pyramid producers (pyramid_kernels.hip) run unchanged on the same bytes.
//   intensity  u8 gray / RGB / BGR              -> packed u8 gray
//   depth      u16                              -> packed u16 (the producers apply the scale, as for a host u16 upload)
//              f64                              -> packed f64
//              f32 / f16                        -> packed f64, (double)value * scale: one exact conversion and ONE
//                                                  correctly rounded fp64 multiply (no fused form exists for a lone product)
// One launch per staging chunk and kind; blockIdx.z = frame of the chunk.  Every pixel is read once and written once: the
// kernels are HBM streams and are shaped as such.  Two forms, chosen per launch on the host from the base pointer, the two
// strides and the width (never per pixel):
//   wide    a thread moves one group of pixels with 16-byte loads and 16-byte stores
//           (16 px of u8 / RGB, 8 px of u16 / f16, 4 px of f32, 2 px of f64); needs 16-byte aligned rows and frames and a
//           width that is a whole number of groups
//   scalar  a thread moves one pixel; any stride, any width
// Both flatten (row, group) over blockIdx.x so that narrow images still fill their 256-thread workgroups.

#include <hip/hip_runtime.h>

#include "phovo_internal.hpp"

#pragma clang fp contract(off)

namespace phovo_hip {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// The project's one colour-to-gray rule (apps/io/png_io.cpp, read_gray8): integer arithmetic, so every path agrees exactly.
__device__ __forceinline__ uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b)
{
  return (9797u * r + 19234u * g + 3737u * b + 16384u) >> 15;
}

// byte k of an array of little-endian 32-bit words (k is a compile-time constant after unrolling: no scratch)
template <int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[N], int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu; }

struct PackArgs {
  const unsigned char *src;      // first frame of the chunk in the caller's memory
  size_t row_stride, frame_stride;   // bytes
  unsigned char *dst;            // packed staging: frame f at dst + f * w * h * (bytes per staged pixel)
  int w, h;
  double scale;                  // f32 / f16 depth
};

template <int FORMAT> struct PackTraits;
template <> struct PackTraits<PHOVO_IMAGE_U8_GRAY> { static constexpr int src_px = 1, dst_px = 1, group = 16; };
template <> struct PackTraits<PHOVO_IMAGE_U8_RGB>  { static constexpr int src_px = 3, dst_px = 1, group = 16; };
template <> struct PackTraits<PHOVO_IMAGE_U8_BGR>  { static constexpr int src_px = 3, dst_px = 1, group = 16; };
template <> struct PackTraits<PHOVO_IMAGE_F64>     { static constexpr int src_px = 8, dst_px = 8, group = 2; };
template <> struct PackTraits<PHOVO_IMAGE_F32>     { static constexpr int src_px = 4, dst_px = 8, group = 4; };
template <> struct PackTraits<PHOVO_IMAGE_F16>     { static constexpr int src_px = 2, dst_px = 8, group = 8; };
template <> struct PackTraits<PHOVO_IMAGE_U16>     { static constexpr int src_px = 2, dst_px = 2, group = 8; };

// one group: 16-byte loads from s (16-byte aligned), 16-byte stores to d (16-byte aligned)
template <int FORMAT>
__device__ __forceinline__ void pack_group(const unsigned char *s, unsigned char *d, double scale)
{
  if constexpr (FORMAT == PHOVO_IMAGE_U8_GRAY) {
    *reinterpret_cast<u32x4 *>(d) = *reinterpret_cast<const u32x4 *>(s);
  } else if constexpr (FORMAT == PHOVO_IMAGE_U8_RGB || FORMAT == PHOVO_IMAGE_U8_BGR) {
    const u32x4 a = reinterpret_cast<const u32x4 *>(s)[0], b = reinterpret_cast<const u32x4 *>(s)[1],
                c = reinterpret_cast<const u32x4 *>(s)[2];
    const uint32_t in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 16; p++) {
      const uint32_t c0 = byte_of(in, 3 * p), c1 = byte_of(in, 3 * p + 1), c2 = byte_of(in, 3 * p + 2);
      const uint32_t y = FORMAT == PHOVO_IMAGE_U8_RGB ? gray_of(c0, c1, c2) : gray_of(c2, c1, c0);
      out[p >> 2] |= y << ((p & 3) * 8);
    }
    u32x4 o; o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
    *reinterpret_cast<u32x4 *>(d) = o;
  } else if constexpr (FORMAT == PHOVO_IMAGE_U16) {
    *reinterpret_cast<u16x8 *>(d) = *reinterpret_cast<const u16x8 *>(s);
  } else if constexpr (FORMAT == PHOVO_IMAGE_F64) {
    *reinterpret_cast<f64x2 *>(d) = *reinterpret_cast<const f64x2 *>(s);
  } else if constexpr (FORMAT == PHOVO_IMAGE_F32) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(s);
    f64x2 lo, hi;
    lo.x = (double)v.x * scale; lo.y = (double)v.y * scale;
    hi.x = (double)v.z * scale; hi.y = (double)v.w * scale;
    reinterpret_cast<f64x2 *>(d)[0] = lo;
    reinterpret_cast<f64x2 *>(d)[1] = hi;
  } else {
    static_assert(FORMAT == PHOVO_IMAGE_F16, "format");
    const f16x8 v = *reinterpret_cast<const f16x8 *>(s);
#pragma unroll
    for (int p = 0; p < 4; p++) {
      f64x2 o;
      o.x = (double)(float)v[2 * p] * scale; o.y = (double)(float)v[2 * p + 1] * scale;
      reinterpret_cast<f64x2 *>(d)[p] = o;
    }
  }
}

// one pixel, natural alignment of the element only
template <int FORMAT>
__device__ __forceinline__ void pack_pixel(const unsigned char *s, unsigned char *d, double scale)
{
  if constexpr (FORMAT == PHOVO_IMAGE_U8_GRAY) {
    *d = *s;
  } else if constexpr (FORMAT == PHOVO_IMAGE_U8_RGB) {
    *d = (unsigned char)gray_of(s[0], s[1], s[2]);
  } else if constexpr (FORMAT == PHOVO_IMAGE_U8_BGR) {
    *d = (unsigned char)gray_of(s[2], s[1], s[0]);
  } else if constexpr (FORMAT == PHOVO_IMAGE_U16) {
    *reinterpret_cast<uint16_t *>(d) = *reinterpret_cast<const uint16_t *>(s);
  } else if constexpr (FORMAT == PHOVO_IMAGE_F64) {
    *reinterpret_cast<double *>(d) = *reinterpret_cast<const double *>(s);
  } else if constexpr (FORMAT == PHOVO_IMAGE_F32) {
    *reinterpret_cast<double *>(d) = (double)*reinterpret_cast<const float *>(s) * scale;
  } else {
    static_assert(FORMAT == PHOVO_IMAGE_F16, "format");
    *reinterpret_cast<double *>(d) = (double)(float)*reinterpret_cast<const _Float16 *>(s) * scale;
  }
}

// WIDE: one thread per group of PackTraits::group pixels (a.w is a multiple of it); else one thread per pixel.
// blockIdx.x * 256 + threadIdx.x runs over (row, group-or-pixel of the row); blockIdx.z = frame.
template <int FORMAT, bool WIDE>
__global__ __launch_bounds__(256) void k_ingest_pack(PackArgs a)
{
  using T = PackTraits<FORMAT>;
  constexpr int G = WIDE ? T::group : 1;
  const uint32_t per_row = (uint32_t)a.w / G;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= per_row * (uint32_t)a.h) return;
  const uint32_t row = idx / per_row, col = (idx - row * per_row) * G;
  const size_t f = blockIdx.z;
  const unsigned char *s = a.src + f * a.frame_stride + (size_t)row * a.row_stride + (size_t)col * T::src_px;
  unsigned char *d = a.dst + ((f * (size_t)a.h + row) * (size_t)a.w + col) * T::dst_px;
  if constexpr (WIDE) pack_group<FORMAT>(s, d, a.scale);
  else pack_pixel<FORMAT>(s, d, a.scale);
}

template <int FORMAT>
hipError_t launch_pack(const PackArgs &a, int frames, bool *wide, hipStream_t stream)
{
  using T = PackTraits<FORMAT>;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(a.src) | reinterpret_cast<uintptr_t>(a.dst) | a.row_stride |
                         (frames > 1 ? a.frame_stride : 0) | ((size_t)a.w * (size_t)a.h * T::dst_px);
  *wide = (bits & 15u) == 0 && a.w % T::group == 0;
  const size_t threads = (size_t)(a.w / (*wide ? T::group : 1)) * (size_t)a.h;
  const dim3 grid((unsigned)((threads + 255) / 256), 1, (unsigned)frames);
  if (*wide) hipLaunchKernelGGL((k_ingest_pack<FORMAT, true>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((k_ingest_pack<FORMAT, false>), grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

int ingest_source_pixel_bytes(int format)
{
  switch (format) {
    case PHOVO_IMAGE_U8_GRAY: return 1;
    case PHOVO_IMAGE_U8_RGB: case PHOVO_IMAGE_U8_BGR: return 3;
    case PHOVO_IMAGE_F64: return 8;
    case PHOVO_IMAGE_F32: return 4;
    case PHOVO_IMAGE_F16: case PHOVO_IMAGE_U16: return 2;
    default: return 0;
  }
}

hipError_t ingest_pack(int format, const void *src, size_t row_stride, size_t frame_stride, int frames, int w, int h,
                       double scale, void *dst, bool *wide, hipStream_t stream)
{
  PackArgs a;
  a.src = static_cast<const unsigned char *>(src); a.row_stride = row_stride; a.frame_stride = frame_stride;
  a.dst = static_cast<unsigned char *>(dst); a.w = w; a.h = h; a.scale = scale;
  switch (format) {
    case PHOVO_IMAGE_U8_GRAY: return launch_pack<PHOVO_IMAGE_U8_GRAY>(a, frames, wide, stream);
    case PHOVO_IMAGE_U8_RGB: return launch_pack<PHOVO_IMAGE_U8_RGB>(a, frames, wide, stream);
    case PHOVO_IMAGE_U8_BGR: return launch_pack<PHOVO_IMAGE_U8_BGR>(a, frames, wide, stream);
    case PHOVO_IMAGE_F64: return launch_pack<PHOVO_IMAGE_F64>(a, frames, wide, stream);
    case PHOVO_IMAGE_F32: return launch_pack<PHOVO_IMAGE_F32>(a, frames, wide, stream);
    case PHOVO_IMAGE_F16: return launch_pack<PHOVO_IMAGE_F16>(a, frames, wide, stream);
    case PHOVO_IMAGE_U16: return launch_pack<PHOVO_IMAGE_U16>(a, frames, wide, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace phovo_hip
