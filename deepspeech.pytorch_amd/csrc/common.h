// Shared helpers for the libds2hip kernels (gfx950 / CDNA4 only).
//
// Conventions (see include/ds2hip.h):
//   * every entry point is extern "C", returns ds2_status_t, enqueues work on
//     the caller's stream and never allocates, synchronises or throws;
//   * device buffers are caller-owned; scratch comes in through (ws, ws_bytes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/ds2hip.h"
#include "../../include/ds2hip_test.h"   // the DS2_RUNG_* values of RnnLaunchRec

namespace ds2 {

// Wave width is fixed at 64 on CDNA; never use warpSize-derived 32 idioms.
constexpr int kWave = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

inline hipStream_t as_stream(ds2_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Records the last HIP error string for ds2_last_error().
void set_last_error(const char* where, hipError_t e);
void set_last_error_text(const char* where, const char* what);

inline ds2_status_t launch_status(const char* where) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(where, e);
    return DS2_HIP_ERROR;
  }
  return DS2_OK;
}

// What the recurrent entry point last called on this thread launched (ds2_test_rnn_last_launch,
// include/ds2hip_test.h; rung = its DS2_RUNG_* value).  Host only and thread-local as the
// error string: rnn_rec_reset at the entry point, rnn_rec_launch after every launch that
// went out -- the first one sets the fields, each one counts.
struct RnnLaunchRec {
  int rung, k, c, bts, launches, grid, same_xcd;
};
RnnLaunchRec& rnn_rec();
inline void rnn_rec_reset() { rnn_rec() = RnnLaunchRec{0, 0, 0, 0, 0, 0, 0}; }
inline void rnn_rec_launch(int rung, int k, int c, int bts, int grid, int same_xcd) {
  RnnLaunchRec& r = rnn_rec();
  if (r.launches++ == 0) {
    r.rung = rung;
    r.k = k;
    r.c = c;
    r.bts = bts;
    r.grid = grid;
    r.same_xcd = same_xcd;
  }
}

inline int cdiv(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// log(exp(a) + exp(b)) with -inf handling (CTC recursions).
__device__ __forceinline__ float log_add(float a, float b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  float m = fmaxf(a, b);
  return m + log1pf(expf(-fabsf(a - b)));
}

// log(exp(a) + exp(b)) on the hardware v_exp_f32 / v_log_f32 (about 1 ulp each): the CTC
// alpha/beta recursions are a dependent chain of these, and log1pf/expf cost ~10x the
// instructions.  log(1 + x) for x = exp(-|a - b|) <= 1 loses only terms below ulp(m).
__device__ __forceinline__ float log_add_fast(float a, float b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const float m = fmaxf(a, b);
  return m + __logf(1.0f + __expf(-fabsf(a - b)));
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// Gate nonlinearities on v_exp_f32 / v_rcp_f32 (absolute error ~1e-7) for the recurrences'
// per-step critical path; tanh(x) = 1 - 2 / (1 + e^{2x}) saturates correctly at +-inf.
__device__ __forceinline__ float sigmoid_fast(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float tanh_fast(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
}

}  // namespace ds2
