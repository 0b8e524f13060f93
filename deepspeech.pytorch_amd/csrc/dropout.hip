// Dropout of the Wav2Letter blocks (ref model.py:535-536) on a counter-based Philox4x32-10
// stream -- no mask tensor, the backward regenerates or reads it off the stored output:
//   ds2_dropout_apply          the general op (any c, any alignment; also its own backward)
//   ds2_bn_dropout_apply_amax  BatchNorm affine [+ ReLU] + dropout + row / column maxima of the
//                              stored y in one pass: amax_rc.h's rows_amax_kernel with DROP
//   ds2_bn_relu_dropout_bwd    ds2_bn_relu_bwd with the scale folded into its mask pass
// The element -> (counter, word) mapping is the one written in include/ds2hip.h.
#include "amax_rc.h"

#include <math.h>

namespace ds2 {
namespace {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned ew_grid(int64_t total) {   // grid of a grid-stride elementwise kernel
  const int64_t g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// p in [0, 1] (NaN fails both comparisons)
inline bool valid_p(float p) { return p >= 0.f && p <= 1.f; }

// p < 1.  thr in double: p 2^32 is exact there, so P(drop) = thr / 2^32 lies within 2^-32 of p
inline DropArgs drop_args(float p, uint64_t seed, uint64_t offset) {
  DropArgs d;
  d.thr = (unsigned)floor((double)p * 4294967296.0);
  d.scale = 1.0f / (1.0f - p);
  d.seed_lo = (unsigned)seed;
  d.seed_hi = (unsigned)(seed >> 32);
  d.off_lo = (unsigned)offset;
  d.off_hi = (unsigned)(offset >> 32);
  return d;
}

// One thread per group of four consecutive elements of the flat array: a float4 when VEC (x
// and y 16-B aligned) and the group is whole, else element by element (the tail group, or
// every group of an unaligned operand).  x and y may alias.
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float* x, int64_t total, DropArgs d,
                                                      float* y) {
  const int64_t groups = (total + 3) / 4;
  for (int64_t g = blockIdx.x * 256ll + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i0 = g * 4;
    if (VEC && i0 + 4 <= total) {
      reinterpret_cast<float4*>(y)[g] = drop4(d, g, reinterpret_cast<const float4*>(x)[g]);
    } else {
      const uint4 w = drop_words(d, g);
      const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < total) y[i0 + j] = ws[j] < d.thr ? 0.f : x[i0 + j] * d.scale;
    }
  }
}

// dz = dy * scale where the stored output passed the ReLU and was kept (y > 0), else 0
__global__ __launch_bounds__(256) void relu_drop_mask_kernel(const float* __restrict__ dy,
                                                             const float* __restrict__ y,
                                                             int64_t total, float scale,
                                                             float* __restrict__ dz) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    dz[i] = y[i] > 0.f ? dy[i] * scale : 0.f;
}

}  // namespace
}  // namespace ds2

using namespace ds2;

extern "C" {

ds2_status_t ds2_dropout_apply(const float* x, int rows, int c, float p, uint64_t seed,
                               uint64_t offset, float* y, ds2_stream_t stream) {
  if (rows < 0 || c < 0 || !valid_p(p)) return DS2_INVALID_VALUE;
  const int64_t total = (int64_t)rows * c;
  if (total == 0) return DS2_OK;
  hipStream_t st = as_stream(stream);
  if (p == 1.f) {
    (void)hipMemsetAsync(y, 0, (size_t)total * 4, st);
    return launch_status("ds2_dropout_apply");
  }
  const DropArgs d = drop_args(p, seed, offset);
  const dim3 grid(ew_grid((total + 3) / 4));
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0)
    hipLaunchKernelGGL(dropout_kernel<true>, grid, dim3(256), 0, st, x, total, d, y);
  else
    hipLaunchKernelGGL(dropout_kernel<false>, grid, dim3(256), 0, st, x, total, d, y);
  return launch_status("ds2_dropout_apply");
}

ds2_status_t ds2_bn_dropout_apply_amax(const float* x, int rows, int c, const float* mean,
                                       const float* invstd, const float* gamma,
                                       const float* beta, int relu, float p, uint64_t seed,
                                       uint64_t offset, float* y, unsigned* row_amax,
                                       unsigned* col_amax, ds2_stream_t stream) {
  if (rows < 0 || c < 0 || !valid_p(p)) return DS2_INVALID_VALUE;
  if (row_amax == nullptr || col_amax == nullptr) return DS2_INVALID_VALUE;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) |
                         reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(invstd) |
                         reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta);
  if (c % 4 != 0 || c > 2048 || (bits & 15) != 0) return DS2_UNSUPPORTED_SHAPE;
  if (rows == 0 || c == 0) return DS2_OK;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(col_amax, 0, (size_t)c * 4, st) != hipSuccess)
    return launch_status("ds2_bn_dropout_apply_amax");
  if (p == 1.f) {   // everything dropped: y and both maxima are zero
    (void)hipMemsetAsync(y, 0, (size_t)rows * c * 4, st);
    (void)hipMemsetAsync(row_amax, 0, (size_t)rows * 4, st);
    return launch_status("ds2_bn_dropout_apply_amax");
  }
  const DropArgs d = drop_args(p, seed, offset);
  if (relu)
    launch_rows_amax<true, true, true>(x, rows, c, c, mean, invstd, gamma, beta, y, row_amax,
                                       col_amax, st, d);
  else
    launch_rows_amax<true, false, true>(x, rows, c, c, mean, invstd, gamma, beta, y, row_amax,
                                        col_amax, st, d);
  return launch_status("ds2_bn_dropout_apply_amax");
}

ds2_status_t ds2_bn_relu_dropout_bwd(const float* dy, const float* y, const float* x, int rows,
                                     int c, const float* mean, const float* invstd,
                                     const float* gamma, const float* beta, float p, float* dx,
                                     float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                     ds2_stream_t stream) {
  if (rows < 0 || c < 0 || !valid_p(p)) return DS2_INVALID_VALUE;
  const int64_t total = (int64_t)rows * c;
  if (total == 0) return DS2_OK;
  if (ws == nullptr || ws_bytes < ds2_bn_relu_bwd_workspace_size(rows, c))
    return DS2_WORKSPACE_TOO_SMALL;
  float* dz = static_cast<float*>(ws);
  const size_t off = al256((size_t)total * 4);
  // p == 1: y is all zero, so the (infinite) scale is never multiplied in
  hipLaunchKernelGGL(relu_drop_mask_kernel, dim3(ew_grid(total)), dim3(256), 0, as_stream(stream),
                     dy, y, total, 1.0f / (1.0f - p), dz);
  const ds2_status_t e = launch_status("ds2_bn_relu_dropout_bwd");
  if (e != DS2_OK) return e;
  return ds2_bn_backward(dz, 0, x, rows, c, 1, 1, mean, invstd, gamma, beta, 0, nullptr, 0.f, 0.f,
                         /*eps: not known here, the stored invstd at every count*/ 0.f, dx, dgamma,
                         dbeta, nullptr, static_cast<char*>(ws) + off, ws_bytes - off, stream);
}

}  // extern "C"
