// The per-frame arithmetic of the spectrogram kernels, shared by stft.hip (whole utterances)
// and stft_stream.hip (PCM chunks): a frame's value depends on its own n_fft samples and its
// bin only, so both files get the same bits for it by running the same code -- the windowed
// tap window[m] * (double)y, the fp64 FMA chain over m = 0 .. n_fft - 1 with twiddles from
// sincospi, hypotf of the float casts, log1pf(mag * gain), and the float32 mean over the rows.
#pragma once

#include "common.h"

namespace ds2 {

constexpr int SMAXN = 1024;    // max n_fft
constexpr int kRows = 161;     // rows of the returned spectrogram (data_loader_aug.py:234-249)

__device__ __forceinline__ int reflect_idx(int i, int n) {
  // numpy 'reflect' (edge sample not repeated); one sample is repeated everywhere
  if (n <= 1) return 0;
  const int period = 2 * (n - 1);
  i = i % period;
  if (i < 0) i += period;
  return i < n ? i : period - i;
}

// librosa's frame count with center=True: the signal padded by n_fft/2 on both sides holds
// 1 + (n + 2 (n_fft/2) - n_fft) / hop frames -- for odd n_fft that is 1 + (n - 1) / hop.  A row
// without samples has no frames (np.pad cannot reflect an empty axis; the host refuses it).
__device__ __forceinline__ int frame_count(int n, int n_fft, int hop) {
  return n >= 1 ? 1 + (n + 2 * (n_fft / 2) - n_fft) / hop : 0;
}

// cs[m], sn[m] = cos, sin(2 pi m / n_fft): the table the DFT indexes by (k m) mod n_fft
__device__ __forceinline__ void stft_twiddles(double* cs, double* sn, int n_fft) {
  for (int m = threadIdx.x; m < n_fft; m += blockDim.x) {
    double s, c;
    sincospi(2.0 * m / n_fft, &s, &c);
    cs[m] = c;
    sn[m] = s;
  }
}

__device__ __forceinline__ double stft_tap(const double* __restrict__ window, int m, float y) {
  return window[m] * (double)y;
}

// bin k of NF frames (fr[f][m], windowed): one serial FMA chain per frame and part
template <int NF>
__device__ __forceinline__ void stft_dft(const double* cs, const double* sn,
                                         const double (*fr)[SMAXN], int n_fft, int k,
                                         double (&re)[NF], double (&im)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) { re[f] = 0.0; im[f] = 0.0; }
  int idx = 0;   // (k * m) mod n_fft
  for (int m = 0; m < n_fft; ++m) {
    const double c = cs[idx], s = sn[idx];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const double v = fr[f][m];
      re[f] = fma(v, c, re[f]);
      im[f] = fma(-v, s, im[f]);
    }
    idx += k;
    if (idx >= n_fft) idx -= n_fft;
  }
}

__device__ __forceinline__ float stft_mag(double re, double im) {
  return hypotf(static_cast<float>(re), static_cast<float>(im));
}

__device__ __forceinline__ float stft_logmag(float mag, float gain) { return log1pf(mag * gain); }

// Sum over the block's 256 threads of every frame's value, one partial per wave into
// red[f][wave]; after a barrier stft_frame_mean(red[f], R) is the frame's mean over R rows.
template <int NF>
__device__ __forceinline__ void stft_frame_sums(const double (&lsum)[NF], double (*red)[4]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    double v = wave_sum_d(lsum[f]);
    if ((threadIdx.x & 63) == 0) red[f][threadIdx.x >> 6] = v;
  }
}

__device__ __forceinline__ double stft_frame_sum(const double* red4) {
  return red4[0] + red4[1] + red4[2] + red4[3];
}

}  // namespace ds2
