// Streaming spectrogram front-end: PCM chunks -> the frames of stft.hip that have become
// final (ds2_stft_stream_*; ds2amd.streaming.StreamingFrontend).
//
// Geometry is stft.hip's (librosa center=True): pad = n_fft / 2, frame t reads the padded
// samples t hop .. t hop + n_fft - 1, i.e. samples t hop - pad + m, reflected at both ends.
// With a samples arrived and the utterance open, frame t is final iff its right edge
// t hop - pad + n_fft - 1 and, for the first frames, the sample its left reflection reads,
// pad - t hop, are both <= a - 1.  The larger of the two is pad for t = 0 and the right edge
// from t = 1 on, and it grows with t, so the final frames are the first
//   a >= pad + 1 ? 1 + (a + pad - n_fft) / hop : 0
// and a final frame reads reflect_idx(i, a') = reflect_idx(i, a) for every later length a'.
// The last feed (last = 1) emits the rest up to librosa's count with the right reflection at
// the true end; for a <= pad that is every frame, the left reflection folding as well.
//
// A frame's bits are those of stft_kernel: both run stft_frame.h on the frame's n_fft samples.
//
// Carried per stream (one record of the caller's state buffer): the last min(a, n_fft - 1)
// samples -- every sample a frame that is not final yet can read directly or through the
// right reflection (which reaches back to a - 1 - pad >= a - n_fft + 1) -- and samples
// 0 .. pad, which the left reflection of the first frames reads; the fp64 sum of the frame
// means and the prior of the causal offset; a tag (magic, n_fft, hop, samples taken) without
// which a record is not advanced.  Samples are kept as the float32 the DFT reads, so int16
// input is converted once, in the kernel that reads it.
//
// Two launches per feed: stft_stream_kernel (the DFT of the k new frames over carried-plus-new
// samples; writes val = log1p(|X| gain), minus the fixed offset if one is given, and every
// frame's mean) and stft_stream_tail_kernel (one block per stream: the running sum in frame
// order, the causal offsets and their subtraction, the new tail and tag).
#include "common.h"
#include "stft_frame.h"

#ifndef DS2_STREAM_SF
#define DS2_STREAM_SF 2
#endif

namespace ds2 {

constexpr int SSF = DS2_STREAM_SF;         // frames per stft_stream_kernel block
constexpr int kStreamMagic = 0x53544654;   // 'STFT'
constexpr int kScan = 256;                 // frames per tile of the offset scan

struct StreamRec {       // the head of a record; head[pad + 1] and tail[n_fft - 1] floats follow
  int magic, n_fft, hop, reserved;
  long long samples;     // samples taken since init
  double sum;            // S_t: sum of the frame means so far, in frame order
  double prior_o0, prior_w, prior_sum;   // the prior (o0, w) and w o0
  double spare;
};
static_assert(sizeof(StreamRec) == 64, "record header");

__host__ __device__ inline size_t stream_rec_bytes(int n_fft) {
  const size_t b = sizeof(StreamRec) + sizeof(float) * (size_t)((n_fft / 2 + 1) + (n_fft - 1));
  return (b + 255) & ~(size_t)255;
}

__device__ __forceinline__ bool stream_rec_ok(const StreamRec* r, int n_fft, int hop, int done) {
  return r->magic == kStreamMagic && r->n_fft == n_fft && r->hop == hop && r->samples == done;
}

// sample j (0 <= j < done + chunk_samples) of stream b: from the chunk, the carried tail or
// the carried head.  chunk points at the stream's row.
__device__ __forceinline__ float stream_sample(int j, int done, int n_fft, const void* chunk,
                                               int dtype, float scale, const float* head,
                                               const float* tail) {
  if (j >= done) {
    if (dtype == 1) return (float)static_cast<const short*>(chunk)[j - done] * scale;
    return static_cast<const float*>(chunk)[j - done];
  }
  const int tail_start = done > n_fft - 1 ? done - (n_fft - 1) : 0;
  if (j >= tail_start) return tail[j - tail_start];
  const int pad = n_fft / 2;
  return head[j < pad ? j : pad];
}

// grid (ceil(k / NF), n); block 256 (thread = frequency bin).  Frames t_first .. t_first + k - 1
// over the done carried and chunk_samples new samples.
template <int NF>
__global__ __launch_bounds__(256) void stft_stream_kernel(
    const void* __restrict__ chunk, int dtype, long long chunk_stride, float scale,
    int chunk_samples, int done, int n_fft, int hop, const double* __restrict__ window,
    int normalize, const float* __restrict__ fixed_offset, const char* __restrict__ state,
    long long rec_bytes, float* __restrict__ out, int k, int t_first,
    float* __restrict__ frame_mean) {
  __shared__ double cs[SMAXN], sn[SMAXN];
  __shared__ double fr[NF][SMAXN];
  __shared__ double red[NF][4];
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * NF;
  const char* recp = state + (long long)b * rec_bytes;
  const StreamRec* rec = reinterpret_cast<const StreamRec*>(recp);
  if (!stream_rec_ok(rec, n_fft, hop, done)) return;   // the tail kernel reports it
  const int pad = n_fft / 2;
  const float* head = reinterpret_cast<const float*>(recp + sizeof(StreamRec));
  const float* tail = head + pad + 1;
  const int a = done + chunk_samples;
  const char* row =
      static_cast<const char*>(chunk) + (long long)b * chunk_stride * (dtype == 1 ? 2 : 4);
  stft_twiddles(cs, sn, n_fft);
  for (int i = threadIdx.x; i < NF * n_fft; i += blockDim.x) {
    const int f = i / n_fft;
    const int m = i - f * n_fft;
    double v = 0.0;
    if (f0 + f < k) {
      const int j = reflect_idx((t_first + f0 + f) * hop + m - pad, a);
      v = stft_tap(window, m, stream_sample(j, done, n_fft, row, dtype, scale, head, tail));
    }
    fr[f][m] = v;
  }
  __syncthreads();
  const int bin = threadIdx.x;
  double lsum[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) lsum[f] = 0.0;
  const float gain = normalize == 1 ? 1048576.0f : 1.0f;
  if (bin < kRows) {
    double re[NF], im[NF];
    stft_dft<NF>(cs, sn, fr, n_fft, bin, re, im);
    const bool fixed = fixed_offset != nullptr;
    const float off = fixed ? fixed_offset[b] : 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      if (f0 + f >= k) continue;
      const float val = stft_logmag(stft_mag(re[f], im[f]), gain);
      lsum[f] = val;
      out[((long long)b * kRows + bin) * k + f0 + f] = fixed ? val - off : val;
    }
  }
  if (frame_mean == nullptr) return;
  stft_frame_sums<NF>(lsum, red);
  __syncthreads();
  if (threadIdx.x < NF && f0 + threadIdx.x < k)
    frame_mean[(long long)b * k + f0 + threadIdx.x] =
        static_cast<float>(stft_frame_sum(red[threadIdx.x]) / kRows);
}

// grid n; block 256.  Per stream: S_t = S_{t-1} + (double)m_t in frame order, the causal
// offsets off_t = (w o0 + S_t) / (w + t + 1) and out -= (float)off_t (subtract != 0), then the
// carried samples and the tag for the next feed.
__global__ __launch_bounds__(256) void stft_stream_tail_kernel(
    const void* __restrict__ chunk, int dtype, long long chunk_stride, float scale,
    int chunk_samples, int done, int n_fft, int hop, char* __restrict__ state,
    long long rec_bytes, float* __restrict__ out, int k, int t_first,
    float* __restrict__ frame_mean, int subtract, double* __restrict__ cur_offset,
    int* __restrict__ out_frames) {
  __shared__ double ps[kScan];
  __shared__ float stage[SMAXN];
  __shared__ double carry;
  const int b = blockIdx.x;
  char* recp = state + (long long)b * rec_bytes;
  StreamRec* rec = reinterpret_cast<StreamRec*>(recp);
  if (!stream_rec_ok(rec, n_fft, hop, done)) {
    if (threadIdx.x == 0 && out_frames != nullptr) out_frames[b] = -1;
    return;
  }
  const int pad = n_fft / 2;
  float* head = reinterpret_cast<float*>(recp + sizeof(StreamRec));
  float* tail = head + pad + 1;
  const double pw = rec->prior_w, psum = rec->prior_sum;
  if (threadIdx.x == 0) carry = rec->sum;
  if (frame_mean != nullptr) {
    float* fm = frame_mean + (long long)b * k;
    for (int base = 0; base < k; base += kScan) {
      const int cnt = k - base < kScan ? k - base : kScan;
      if (threadIdx.x < cnt) ps[threadIdx.x] = (double)fm[base + threadIdx.x];
      __syncthreads();
      if (threadIdx.x == 0) {
        double s = carry;
        for (int i = 0; i < cnt; ++i) {
          s += ps[i];
          ps[i] = s;
        }
        carry = s;
      }
      __syncthreads();
      if (threadIdx.x < cnt)
        fm[base + threadIdx.x] = static_cast<float>(
            (psum + ps[threadIdx.x]) / (pw + (double)(t_first + base + threadIdx.x + 1)));
      __syncthreads();
    }
    if (subtract) {
      float* o = out + (long long)b * kRows * k;
      for (int i = threadIdx.x; i < kRows * k; i += blockDim.x) o[i] -= fm[i % k];
    }
  }
  // the samples the next feed still reads: the last min(a, n_fft - 1), staged so that the
  // old tail is read before it is overwritten; samples 0 .. pad when they arrive
  const int a = done + chunk_samples;
  const char* row =
      static_cast<const char*>(chunk) + (long long)b * chunk_stride * (dtype == 1 ? 2 : 4);
  const int new_start = a > n_fft - 1 ? a - (n_fft - 1) : 0;
  const int keep = a - new_start;
  for (int i = threadIdx.x; i < keep; i += blockDim.x)
    stage[i] = stream_sample(new_start + i, done, n_fft, row, dtype, scale, head, tail);
  __syncthreads();
  for (int i = threadIdx.x; i < keep; i += blockDim.x) tail[i] = stage[i];
  const int head_end = a < pad + 1 ? a : pad + 1;
  for (int j = done + threadIdx.x; j < head_end; j += blockDim.x)
    head[j] = stream_sample(j, done, n_fft, row, dtype, scale, head, tail);
  if (threadIdx.x == 0) {
    const int frames = t_first + k;
    rec->sum = carry;
    rec->samples = a;
    if (cur_offset != nullptr) cur_offset[b] = frames > 0 ? carry / frames : rec->prior_o0;
    if (out_frames != nullptr) out_frames[b] = frames;
  }
}

__global__ void stft_stream_init_kernel(char* __restrict__ state, long long rec_bytes, int n_fft,
                                        int hop, const double* __restrict__ prior_offset,
                                        double prior_frames) {
  StreamRec* rec = reinterpret_cast<StreamRec*>(state + (long long)blockIdx.x * rec_bytes);
  if (threadIdx.x != 0) return;
  const double o0 = prior_offset != nullptr ? prior_offset[blockIdx.x] : 0.0;
  const double w = prior_offset != nullptr ? prior_frames : 0.0;
  rec->magic = kStreamMagic;
  rec->n_fft = n_fft;
  rec->hop = hop;
  rec->reserved = 0;
  rec->samples = 0;
  rec->sum = 0.0;
  rec->prior_o0 = o0;
  rec->prior_w = w;
  rec->prior_sum = w * o0;
  rec->spare = 0.0;
}

}  // namespace ds2

using namespace ds2;

// frames that are final after a samples: every frame of the utterance if it has ended
static long long stream_frames(long long a, int last, int n_fft, int hop) {
  const int pad = n_fft / 2;
  if (last) return a >= 1 ? 1 + (a + 2 * pad - n_fft) / hop : 0;
  return a >= pad + 1 ? 1 + (a + pad - n_fft) / hop : 0;
}

// DS2_OK where a state exists for the geometry
static ds2_status_t stream_geometry(int n, int n_fft, int hop) {
  if (n < 0 || n_fft < 2 || n_fft > SMAXN || hop < 1) return DS2_INVALID_VALUE;
  // 161 rows need 161 bins: the reference's mirror-fill for fewer reads frames that lie
  // ahead of the column it fills, further ahead the later the column
  if (n_fft / 2 + 1 > 256 || n_fft / 2 + 1 < kRows) return DS2_UNSUPPORTED_SHAPE;
  return DS2_OK;
}

extern "C" {

size_t ds2_stft_stream_state_size(int n, int n_fft, int hop) {
  if (n < 1 || stream_geometry(n, n_fft, hop) != DS2_OK) return 0;
  return (size_t)n * stream_rec_bytes(n_fft);
}

size_t ds2_stft_stream_workspace_size(int n, int k) {
  if (n < 1 || k < 1) return 0;
  return ((size_t)n * k * sizeof(float) + 255) & ~(size_t)255;
}

ds2_status_t ds2_stft_stream_init(void* state, size_t state_bytes, int n, int n_fft, int hop,
                                  const double* prior_offset, double prior_frames,
                                  ds2_stream_t stream) {
  const ds2_status_t g = stream_geometry(n, n_fft, hop);
  if (g != DS2_OK) return g;
  if (n < 1 || !(prior_frames >= 0.0)) return DS2_INVALID_VALUE;
  if (state == nullptr || (reinterpret_cast<uintptr_t>(state) & 255) != 0 ||
      state_bytes < ds2_stft_stream_state_size(n, n_fft, hop))
    return DS2_INVALID_VALUE;
  hipLaunchKernelGGL(stft_stream_init_kernel, dim3(n), dim3(64), 0, as_stream(stream),
                     static_cast<char*>(state), (long long)stream_rec_bytes(n_fft), n_fft, hop,
                     prior_offset, prior_frames);
  return launch_status("ds2_stft_stream_init");
}

ds2_status_t ds2_stft_stream_feed(const void* chunk, int dtype, int n, int chunk_samples,
                                  int64_t chunk_stride, float scale, int64_t samples_done,
                                  int last, int n_fft, int hop, const double* window,
                                  int normalize, const float* fixed_offset, float* out, int k,
                                  double* cur_offset, int* out_frames, void* state,
                                  size_t state_bytes, void* ws, size_t ws_bytes,
                                  ds2_stream_t stream) {
  const ds2_status_t g = stream_geometry(n, n_fft, hop);
  if (g != DS2_OK) return g;
  if (chunk_samples < 0 || samples_done < 0 || k < 0 || (dtype != 0 && dtype != 1) ||
      (last != 0 && last != 1) || (normalize != 0 && normalize != 1) ||
      (n > 1 && chunk_stride < chunk_samples))
    return DS2_INVALID_VALUE;
  if (normalize == 0 && fixed_offset != nullptr) return DS2_INVALID_VALUE;
  // sample indices and t hop are ints in the kernels
  if (samples_done + chunk_samples > (int64_t)INT32_MAX - 2 * SMAXN) return DS2_INVALID_VALUE;
  const long long t_first = stream_frames(samples_done, 0, n_fft, hop);
  if (stream_frames(samples_done + chunk_samples, last, n_fft, hop) - t_first != k)
    return DS2_INVALID_VALUE;
  if (n == 0 || (chunk_samples == 0 && !last)) return DS2_OK;
  if (state == nullptr || (reinterpret_cast<uintptr_t>(state) & 255) != 0 ||
      state_bytes < ds2_stft_stream_state_size(n, n_fft, hop))
    return DS2_INVALID_VALUE;
  if (chunk_samples > 0 && chunk == nullptr) return DS2_INVALID_VALUE;
  if (k > 0 && (window == nullptr || out == nullptr)) return DS2_INVALID_VALUE;
  if ((int64_t)n * kRows * k > INT32_MAX) return DS2_UNSUPPORTED_SHAPE;
  float* frame_mean = nullptr;
  if (k > 0 && normalize == 1) {
    if (ws == nullptr || ws_bytes < ds2_stft_stream_workspace_size(n, k))
      return DS2_WORKSPACE_TOO_SMALL;
    frame_mean = static_cast<float*>(ws);
  }
  hipStream_t st = as_stream(stream);
  const long long rb = (long long)stream_rec_bytes(n_fft);
  const int done = static_cast<int>(samples_done);
  if (k > 0)
    hipLaunchKernelGGL(stft_stream_kernel<SSF>, dim3(cdiv(k, SSF), n), dim3(256), 0, st, chunk,
                       dtype, (long long)chunk_stride, scale, chunk_samples, done, n_fft, hop,
                       window, normalize, fixed_offset, static_cast<const char*>(state), rb, out,
                       k, static_cast<int>(t_first), frame_mean);
  hipLaunchKernelGGL(stft_stream_tail_kernel, dim3(n), dim3(256), 0, st, chunk, dtype,
                     (long long)chunk_stride, scale, chunk_samples, done, n_fft, hop,
                     static_cast<char*>(state), rb, out, k, static_cast<int>(t_first), frame_mean,
                     fixed_offset == nullptr ? 1 : 0, cur_offset, out_frames);
  return launch_status("ds2_stft_stream_feed");
}

}  // extern "C"
