// Waveform augmentations ahead of the STFT: the arithmetic of data/audio_aug.py's Shift
// (:26-44), AudioDistort (:47-60, clip :177-178) and AddNoise (:78-107) as per-utterance
// op lists executed on the device.  The host draws every random number in the
// reference's order (ds2amd/audio_aug.py) and records what each transform does; this
// kernel replays the records:
//   SHIFT   (shift, limit): y[i] = x[i - shift] for shift <= i < shift + len, else 0;
//           len += limit                                  (np.zeros(len + limit) fill)
//   DISTORT (alpha):        y = clip(f32(alpha) * x, 0, max(x))     (float32 numpy math)
//   NOISE   (row, alpha):   y = (x + alpha * noise[row][i]) / (1 + alpha)  in float64
//           (the noise slice noise[pos : pos + len] is cut on the host; float64 like
//           np.random.normal's draws)
// Between ops the samples are kept in fp32 (the STFT input type).  One workgroup per
// utterance: DISTORT needs the utterance's max before any output sample.
#include "common.h"

namespace ds2 {

constexpr int WAV_T = 1024;
enum { WAV_END = 0, WAV_SHIFT = 1, WAV_DISTORT = 2, WAV_NOISE = 3 };

__global__ __launch_bounds__(WAV_T) void wave_aug_kernel(
    const float* __restrict__ in, int64_t in_stride, const int* __restrict__ in_lens,
    const int* __restrict__ op_i, const double* __restrict__ op_f, int max_ops,
    const double* __restrict__ noise, int64_t noise_stride, float* __restrict__ buf, int64_t cap,
    float* __restrict__ out, int64_t out_stride, const int* __restrict__ out_lens,
    int* __restrict__ err) {
  __shared__ float red[WAV_T / kWave];
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  int64_t len = in_lens[n];
  // Consistency word: 1 = a length past cap (the input's, or a SHIFT's result) or a shift
  // outside [0, limit]; 2 = a record that cannot be replayed (unknown kind, NOISE without a
  // noise table); 4 = the final length is not out_lens[n].  A row that sets it writes nothing
  // from that record on, and nothing to out.
  if (len > cap) {
    if (tid == 0) atomicOr(err, 1);
    return;
  }
  const float* src = in + (int64_t)n * in_stride;
  float* pp[2] = {buf + (int64_t)(2 * n) * cap, buf + (int64_t)(2 * n + 1) * cap};
  int which = 0;
  for (int o = 0; o < max_ops; ++o) {
    const int* rec = op_i + ((int64_t)n * max_ops + o) * 4;
    const int kind = rec[0];
    if (kind == WAV_END) break;
    float* dst = pp[which];
    if (kind == WAV_SHIFT) {
      const int64_t shift = rec[1], nl = len + rec[2];
      if (nl > cap || shift < 0 || shift > rec[2]) {
        if (tid == 0) atomicOr(err, 1);
        return;
      }
      for (int64_t i = tid; i < nl; i += WAV_T)
        dst[i] = (i >= shift && i < shift + len) ? src[i - shift] : 0.f;
      len = nl;
    } else if (kind == WAV_DISTORT) {
      float m = -INFINITY;
      for (int64_t i = tid; i < len; i += WAV_T) m = fmaxf(m, src[i]);
      m = wave_max(m);
      if ((tid & 63) == 0) red[tid >> 6] = m;
      __syncthreads();
      m = red[0];
#pragma unroll
      for (int w = 1; w < WAV_T / kWave; ++w) m = fmaxf(m, red[w]);
      const float alpha = static_cast<float>(op_f[(int64_t)n * max_ops + o]);
      // np.clip(v, 0, m) = minimum(maximum(v, 0), m)
      for (int64_t i = tid; i < len; i += WAV_T) dst[i] = fminf(fmaxf(alpha * src[i], 0.f), m);
    } else if (kind == WAV_NOISE) {
      if (noise == nullptr) {
        if (tid == 0) atomicOr(err, 2);
        return;
      }
      const double alpha = op_f[(int64_t)n * max_ops + o];
      const double* nz = noise + (int64_t)rec[1] * noise_stride;
      for (int64_t i = tid; i < len; i += WAV_T)
        dst[i] = static_cast<float>(((double)src[i] + alpha * nz[i]) / (1.0 + alpha));
    } else {
      if (tid == 0) atomicOr(err, 2);
      return;
    }
    __syncthreads();
    src = dst;
    which ^= 1;
  }
  if (len != out_lens[n]) {
    if (tid == 0) atomicOr(err, 4);
    return;
  }
  float* y = out + (int64_t)n * out_stride;
  for (int64_t i = tid; i < out_stride; i += WAV_T) y[i] = i < len ? src[i] : 0.f;
}

// ---------------------------------------------------------------------------------------
// ds2_pcm_decode: the int16 -> float32 arithmetic of load_audio_norm (data/audio_loader.py:4-27,
// scipy wav read + normalise by max |x| + channel selection) on the packed `data` chunks of a
// batch of wav files, so the host uploads 2 bytes per sample and no padding.
//   desc [n][4] int64 = {first int16 element, frames, channels, selector (-1 = mean)}
// Phase 1 (pcm_peak_kernel): abs_max per utterance = max over every sample of every channel of
// np.abs on int16, which wraps: |-32768| = -32768.  Kept as abs_max + 32768 in an unsigned
// word (0 = the smallest value, what the memset leaves) under atomicMax.
// Phase 2 (pcm_scale_kernel): iff abs_max > 0 a sample is (float)((double)s * (1.0 /
// (double)abs_max)): numpy's `sound *= 1 / abs_max` multiplies the float32 array by a float64
// scalar in double and rounds once.  The mean over channels is ndarray.mean(axis=1) in float32:
// a sequential sum for 2..7 channels, numpy's 8-way pairwise tree for 8, one IEEE division.
// Every operation is spelled with the _rn intrinsics: no contraction into an fma.
constexpr int PCM_T = 256;
constexpr int PCM_VEC = 8;        // int16 per 16-byte load
constexpr int PCM_PER_THREAD = 4; // outputs per thread in phase 2
constexpr int PCM_MAX_CH = 8;

// np.abs on int16: the result is wrapped back into int16
__device__ __forceinline__ int pcm_abs16(int s) {
  return static_cast<int>(static_cast<int16_t>(s < 0 ? -s : s));
}

__global__ __launch_bounds__(PCM_T) void pcm_peak_kernel(const int16_t* __restrict__ pcm,
                                                         const int64_t* __restrict__ desc, int bpu,
                                                         unsigned* __restrict__ peak) {
  __shared__ int red[PCM_T / kWave];
  const int b = blockIdx.x / bpu, chunk = blockIdx.x % bpu;
  const int tid = threadIdx.x;
  const int64_t* d = desc + (int64_t)b * 4;
  const int64_t total = d[1] * d[2];
  if (total == 0) return;                      // uniform over the block
  const int16_t* x = pcm + d[0];
  // x is 2-byte aligned and no more (an odd sample count before it): scalar head up to the
  // first 16-byte boundary, 16-byte loads from there, scalar tail
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 1;
  if (head > total) head = total;
  const int64_t nvec = (total - head) / PCM_VEC;
  const int64_t tail0 = head + nvec * PCM_VEC;
  int m = -32768;
  const int4* xv = reinterpret_cast<const int4*>(x + head);
  for (int64_t v = (int64_t)chunk * PCM_T + tid; v < nvec; v += (int64_t)bpu * PCM_T) {
    const int4 q = xv[v];
    const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m = max(m, pcm_abs16(static_cast<int16_t>(w[j] & 0xffff)));
      m = max(m, pcm_abs16(w[j] >> 16));       // arithmetic shift: the sign-extended high half
    }
  }
  if (chunk == 0) {
    for (int64_t i = tid; i < head; i += PCM_T) m = max(m, pcm_abs16(x[i]));
    for (int64_t i = tail0 + tid; i < total; i += PCM_T) m = max(m, pcm_abs16(x[i]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < PCM_T / kWave; ++w) m = max(m, red[w]);
    atomicMax(peak + b, static_cast<unsigned>(m + 32768));
  }
}

__global__ __launch_bounds__(PCM_T) void pcm_scale_kernel(const int16_t* __restrict__ pcm,
                                                          const int64_t* __restrict__ desc,
                                                          const unsigned* __restrict__ peak,
                                                          float* __restrict__ out,
                                                          int64_t out_stride, int cpr) {
  const int b = blockIdx.x / cpr, chunk = blockIdx.x % cpr;
  const int64_t* d = desc + (int64_t)b * 4;
  const int64_t frames = d[1];
  const int ch = static_cast<int>(d[2]), sel = static_cast<int>(d[3]);
  const int16_t* x = pcm + d[0];
  const int abs_max = static_cast<int>(peak[b]) - 32768;
  const bool scaled = abs_max > 0;
  const double scale = scaled ? 1.0 / (double)abs_max : 1.0;
  float* y = out + (int64_t)b * out_stride;
  auto val = [&](int16_t s) -> float {
    return scaled ? __double2float_rn(__dmul_rn((double)s, scale)) : (float)s;
  };
#pragma unroll
  for (int k = 0; k < PCM_PER_THREAD; ++k) {
    const int64_t i = ((int64_t)chunk * PCM_PER_THREAD + k) * PCM_T + threadIdx.x;
    if (i >= out_stride) break;
    float v = 0.f;
    if (i < frames) {
      const int16_t* s = x + i * ch;
      if (ch == 1) {
        v = val(s[0]);
      } else if (sel >= 0) {
        v = val(s[sel]);
      } else if (ch == PCM_MAX_CH) {
        // numpy's pairwise sum over 8 contiguous values
        v = __fadd_rn(__fadd_rn(__fadd_rn(val(s[0]), val(s[1])), __fadd_rn(val(s[2]), val(s[3]))),
                      __fadd_rn(__fadd_rn(val(s[4]), val(s[5])), __fadd_rn(val(s[6]), val(s[7]))));
        v = __fdiv_rn(v, (float)ch);
      } else {
        v = val(s[0]);
        for (int c = 1; c < ch; ++c) v = __fadd_rn(v, val(s[c]));
        v = __fdiv_rn(v, (float)ch);
      }
    }
    y[i] = v;
  }
}

}  // namespace ds2

using namespace ds2;

extern "C" {

size_t ds2_wave_aug_workspace_size(int n, int64_t cap) {
  return n > 0 && cap > 0 ? (size_t)2 * n * cap * sizeof(float) + 256 : 256;
}

ds2_status_t ds2_wave_aug(const float* in, int64_t in_stride, const int* in_lens, int n,
                          const int* op_i, const double* op_f, int max_ops, const double* noise,
                          int64_t noise_stride, float* out, int64_t out_stride,
                          const int* out_lens, int64_t cap, int* err, void* ws, size_t ws_bytes,
                          ds2_stream_t stream) {
  if (n < 0 || max_ops < 0 || in_stride < 0 || out_stride < 0 || cap < 0) return DS2_INVALID_VALUE;
  if (n == 0) return DS2_OK;
  if (in == nullptr || in_lens == nullptr || out == nullptr || out_lens == nullptr ||
      err == nullptr || (max_ops > 0 && (op_i == nullptr || op_f == nullptr)))
    return DS2_INVALID_VALUE;
  if (ws == nullptr || ws_bytes < ds2_wave_aug_workspace_size(n, cap)) return DS2_WORKSPACE_TOO_SMALL;
  hipLaunchKernelGGL(wave_aug_kernel, dim3(n), dim3(WAV_T), 0, as_stream(stream), in, in_stride,
                     in_lens, op_i, op_f, max_ops, noise, noise_stride, static_cast<float*>(ws),
                     cap, out, out_stride, out_lens, err);
  return launch_status("ds2_wave_aug");
}

size_t ds2_pcm_decode_workspace_size(int n) {
  return n > 0 ? (size_t)n * sizeof(unsigned) + 256 : 256;
}

ds2_status_t ds2_pcm_decode(const int16_t* pcm, int64_t pcm_elems, const int64_t* desc_host,
                            const int64_t* desc, int n, float* out, int64_t out_stride, void* ws,
                            size_t ws_bytes, ds2_stream_t stream) {
  if (n < 0 || pcm_elems < 0 || out_stride < 0) return DS2_INVALID_VALUE;
  if (n == 0) return DS2_OK;
  if (desc_host == nullptr || desc == nullptr || out == nullptr) return DS2_INVALID_VALUE;
  if (n > (1 << 20)) return DS2_UNSUPPORTED_SHAPE;
  int64_t max_total = 0;
  for (int b = 0; b < n; ++b) {
    const int64_t off = desc_host[4 * b], frames = desc_host[4 * b + 1];
    const int64_t ch = desc_host[4 * b + 2], sel = desc_host[4 * b + 3];
    if (off < 0 || frames < 0 || ch < 1 || ch > PCM_MAX_CH || sel < -1 || sel >= ch)
      return DS2_INVALID_VALUE;
    if (frames > out_stride || off > pcm_elems || frames > (pcm_elems - off) / ch)
      return DS2_INVALID_VALUE;
    max_total = frames * ch > max_total ? frames * ch : max_total;
  }
  if (max_total > 0 && (pcm == nullptr || (reinterpret_cast<uintptr_t>(pcm) & 1)))
    return DS2_INVALID_VALUE;
  if (ws == nullptr || ws_bytes < ds2_pcm_decode_workspace_size(n)) return DS2_WORKSPACE_TOO_SMALL;
  if (out_stride == 0) return DS2_OK;
  const int64_t cpr64 = (out_stride + PCM_T * PCM_PER_THREAD - 1) / (PCM_T * PCM_PER_THREAD);
  if (cpr64 * n > 0x7fffffffLL) return DS2_UNSUPPORTED_SHAPE;
  hipStream_t st = as_stream(stream);
  unsigned* peak = static_cast<unsigned*>(ws);
  hipError_t e = hipMemsetAsync(peak, 0, (size_t)n * sizeof(unsigned), st);
  if (e != hipSuccess) {
    set_last_error("ds2_pcm_decode", e);
    return DS2_HIP_ERROR;
  }
  if (max_total > 0) {
    // several blocks per utterance: 8192 samples per block and pass, at most 64 blocks
    int bpu = cdiv(max_total, (int64_t)PCM_T * PCM_VEC * 4);
    bpu = bpu < 1 ? 1 : (bpu > 64 ? 64 : bpu);
    hipLaunchKernelGGL(pcm_peak_kernel, dim3((unsigned)n * bpu), dim3(PCM_T), 0, st, pcm, desc,
                       bpu, peak);
  }
  hipLaunchKernelGGL(pcm_scale_kernel, dim3((unsigned)(cpr64 * n)), dim3(PCM_T), 0, st, pcm, desc,
                     peak, out, out_stride, (int)cpr64);
  return launch_status("ds2_pcm_decode");
}

}  // extern "C"
