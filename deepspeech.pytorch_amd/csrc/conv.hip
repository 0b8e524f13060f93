// Conv2d (NCHW, fp32): the extern "C" entry points and the fp32 kernel families, all on
// v_mfma_f32_32x32x2_f32.  ref model.py:208-215: conv1 W[32,1,41,11] s(2,2) p(20,5); conv2
// W[32,32,21,11] s(2,1) p(10,5); MaskConv (model.py:63-79) zeroes output columns w >= len.
//
// An entry point makes the dims, takes the direction's plan (conv_host.h), checks the caller's
// workspace against it and switches on the plan's rung.  The bf16x6 / fp16x3 rungs launch from
// conv_split.hip; here are
//   * the implicit GEMM, which takes every shape, with the slab reduction and the bias
//     gradient of every wgrad rung:
//       fwd  : Y[co][p]  = sum_k W[co][k] * X[k][p]        p = (n, ho, wo) tile of one output row
//       dgrad: DX[ci][q] = sum_k W'[ci][k] * DY[k][q]       q = (n, hi, wi) tile of one input row,
//              k = (co, kh, kw) restricted to the kh of matching stride parity
//       wgrad: DW[co][k] = sum_p DY[co][p] * X[k][p]        split over samples, slab reduce
//     All three stage a [16][32] A tile and a [16][256 or 128] B tile k-major in LDS
//     (conflict-free fragment reads), double-buffered through registers: the gathers of
//     K-step i+1 are in flight while the MFMAs of step i run;
//   * the LDS-patch direct convolution (conv_patch_kernel), the LDS-tile weight gradient
//     (conv_wgrad_patch_kernel: conv1's) and the one-input-channel forward
//     (conv1_patch_fwd_kernel: conv1's).
#include "conv_host.h"

namespace ds2 {

constexpr int CBK = 16;       // K per stage
constexpr int CBN = 256;      // positions per workgroup (fwd / dgrad)
constexpr int CBNW = 128;     // k-columns per workgroup (wgrad)

// ---------------------------------------------------------------------------
// forward. grid (ceil(Wo/256), Ho, N * ceil(Co/32)); block 256 (4 waves, each
// 32 co x 64 positions = 2 MFMA tiles).
__global__ __launch_bounds__(256) void conv_fwd_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ bias,
                                                       float* __restrict__ y, ConvDims g,
                                                       const int* __restrict__ out_lens) {
  __shared__ float As[2][CBK][32];
  __shared__ float Bs[2][CBK][CBN];
  const int cob = (g.co + 31) / 32;
  const int n = blockIdx.z / cob;
  const int co0 = (blockIdx.z - n * cob) * 32;
  const int ho = blockIdx.y;
  const int wo0 = blockIdx.x * CBN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int K = g.ci * g.kh * g.kw;
  const int KHW = g.kh * g.kw;

  const int wo = wo0 + tid;           // this thread's B column
  const int wi_base = wo * g.sw - g.pw;
  const int hi_base = ho * g.sh - g.ph;
  const float* xn = x + (int64_t)n * g.ci * g.hi * g.wi;

  float rb[CBK], ra[2];
  auto load = [&](int k0) {
    // (ci, kh, kw) of k0 once (wave-uniform), then stepped: no per-element division
    int ci = k0 / KHW;
    int khh = (k0 - ci * KHW) / g.kw;
    int kww = k0 - ci * KHW - khh * g.kw;
#pragma unroll
    for (int kk = 0; kk < CBK; ++kk) {
      const int k = k0 + kk;
      float v = 0.f;
      const int hi = hi_base + khh;
      const int wi = wi_base + kww;
      if (k < K && wo < g.wo && hi >= 0 && hi < g.hi && wi >= 0 && wi < g.wi)
        v = xn[((int64_t)ci * g.hi + hi) * g.wi + wi];
      rb[kk] = v;
      if (++kww == g.kw) { kww = 0; if (++khh == g.kh) { khh = 0; ++ci; } }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 256 * q;      // 512 = 16 k x 32 co
      const int kk = e & 15;
      const int c = e >> 4;
      const int k = k0 + kk;
      ra[q] = (k < K && co0 + c < g.co) ? w[(int64_t)(co0 + c) * K + k] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int kk = 0; kk < CBK; ++kk) Bs[buf][kk][tid] = rb[kk];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 256 * q;
      As[buf][e & 15][e >> 4] = ra[q];
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  const int lr = lane & 31, lk = lane >> 5;
  const int wn = wave * 64;
  const int nk = (K + CBK - 1) / CBK;
  load(0);
  store(0);
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int cur = it & 1;
    if (it + 1 < nk) load((it + 1) * CBK);
#pragma unroll
    for (int kk = 0; kk < CBK; kk += 2) {
      const float a = As[cur][kk + lk][lr];
      const float b0 = Bs[cur][kk + lk][wn + lr];
      const float b1 = Bs[cur][kk + lk][wn + 32 + lr];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
    if (it + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }
  const int len = out_lens != nullptr ? out_lens[n] : g.wo;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wo0 + wn + 32 * j + lr;
    if (col >= g.wo) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = co0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (c < g.co) {
        float v = (j == 0 ? acc0[r] : acc1[r]) + (bias != nullptr ? bias[c] : 0.f);
        if (col >= len) v = 0.f;
        y[(((int64_t)n * g.co + c) * g.ho + ho) * g.wo + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dgrad. grid (ceil(Wi/256), Hi, N * ceil(Ci/32)).
__global__ __launch_bounds__(256) void conv_dgrad_kernel(const float* __restrict__ dy,
                                                         const float* __restrict__ w,
                                                         float* __restrict__ dx, ConvDims g) {
  __shared__ float As[2][CBK][32];
  __shared__ float Bs[2][CBK][CBN];
  const int cib = (g.ci + 31) / 32;
  const int n = blockIdx.z / cib;
  const int ci0 = (blockIdx.z - n * cib) * 32;
  const int hi = blockIdx.y;
  const int wi0 = blockIdx.x * CBN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // valid kh: (hi + ph - kh) % sh == 0 and 0 <= (hi + ph - kh)/sh < ho
  const int kh_first = (hi + g.ph) % g.sh;
  const int nkh = kh_first < g.kh ? (g.kh - kh_first + g.sh - 1) / g.sh : 0;
  const int K = g.co * nkh * g.kw;
  const int KHW = nkh * g.kw;
  const int wi = wi0 + tid;
  const float* dyn = dy + (int64_t)n * g.co * g.ho * g.wo;

  float rb[CBK], ra[2];
  auto load = [&](int k0) {
    int c = K > 0 ? k0 / KHW : 0;
    int khi = K > 0 ? (k0 - c * KHW) / g.kw : 0;
    int kww = K > 0 ? k0 - c * KHW - khi * g.kw : 0;
#pragma unroll
    for (int kk = 0; kk < CBK; ++kk) {
      const int k = k0 + kk;
      float v = 0.f;
      const int khh = kh_first + khi * g.sh;
      const int hnum = hi + g.ph - khh;             // divisible by sh by construction
      const int hq = hnum / g.sh;
      const int wnum = wi + g.pw - kww;
      if (k < K && wi < g.wi && hnum >= 0 && hq < g.ho && wnum >= 0) {
        if (g.sw == 1) {
          if (wnum < g.wo) v = dyn[((int64_t)c * g.ho + hq) * g.wo + wnum];
        } else if ((wnum % g.sw) == 0) {
          const int wq = wnum / g.sw;
          if (wq < g.wo) v = dyn[((int64_t)c * g.ho + hq) * g.wo + wq];
        }
      }
      rb[kk] = v;
      if (++kww == g.kw) { kww = 0; if (++khi == nkh) { khi = 0; ++c; } }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 256 * q;
      const int kk = e & 15;
      const int cc = e >> 4;
      const int k = k0 + kk;
      float v = 0.f;
      if (k < K && ci0 + cc < g.ci) {
        const int c = k / KHW;
        const int r = k - c * KHW;
        const int khi = r / g.kw;
        const int kww = r - khi * g.kw;
        const int khh = kh_first + khi * g.sh;
        v = w[(((int64_t)c * g.ci + ci0 + cc) * g.kh + khh) * g.kw + kww];
      }
      ra[q] = v;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int kk = 0; kk < CBK; ++kk) Bs[buf][kk][tid] = rb[kk];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 256 * q;
      As[buf][e & 15][e >> 4] = ra[q];
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  const int lr = lane & 31, lk = lane >> 5;
  const int wn = wave * 64;
  const int nk = (K + CBK - 1) / CBK;
  if (nk > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int cur = it & 1;
    if (it + 1 < nk) load((it + 1) * CBK);
#pragma unroll
    for (int kk = 0; kk < CBK; kk += 2) {
      const float a = As[cur][kk + lk][lr];
      const float b0 = Bs[cur][kk + lk][wn + lr];
      const float b1 = Bs[cur][kk + lk][wn + 32 + lr];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
    if (it + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wi0 + wn + 32 * j + lr;
    if (col >= g.wi) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = ci0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (c < g.ci) dx[(((int64_t)n * g.ci + c) * g.hi + hi) * g.wi + col] = j == 0 ? acc0[r] : acc1[r];
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad partials. grid (ceil(Kc/128), N, ceil(Co/32)); block 256 (4 waves, each
// 32 co x 32 k-columns).  Reduction over (ho, wo) of one sample in steps of 16
// consecutive wo inside one output row.  partial[n][co][Kc].
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ dy,
                                                         const float* __restrict__ x,
                                                         float* __restrict__ partial,
                                                         ConvDims g) {
  __shared__ float As[2][CBK][32];
  __shared__ float Bs[2][CBK][CBNW];
  const int kc0 = blockIdx.x * CBNW;
  const int n = blockIdx.y;
  const int co0 = blockIdx.z * 32;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int Kc = g.ci * g.kh * g.kw;
  const int KHW = g.kh * g.kw;
  // this thread's B column and its (ci, kh, kw)
  const int bcol = tid & (CBNW - 1);
  const int bq = tid >> 7;     // 0..1 -> positions bq*8 .. bq*8+7
  const int kcol = kc0 + bcol;
  int ci = 0, khh = 0, kww = 0;
  const bool kvalid = kcol < Kc;
  if (kvalid) {
    ci = kcol / KHW;
    const int r = kcol - ci * KHW;
    khh = r / g.kw;
    kww = r - khh * g.kw;
  }
  const float* xn = x + ((int64_t)n * g.ci + ci) * g.hi * g.wi;
  const float* dyn = dy + (int64_t)n * g.co * g.ho * g.wo;
  const int wtiles = (g.wo + CBK - 1) / CBK;
  const int nsteps = g.ho * wtiles;

  float rb[8], ra[2];
  auto load = [&](int step) {
    const int ho = step / wtiles;
    const int wo0 = (step - ho * wtiles) * CBK;
    const int hi = ho * g.sh - g.ph + khh;
    const bool hok = kvalid && hi >= 0 && hi < g.hi;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int pp = bq * 8 + i;
      const int wo = wo0 + pp;
      const int wi = wo * g.sw - g.pw + kww;
      float v = 0.f;
      if (hok && wo < g.wo && wi >= 0 && wi < g.wi) v = xn[(int64_t)hi * g.wi + wi];
      rb[i] = v;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 256 * q;     // 16 positions x 32 co, position fastest
      const int pp = e & 15;
      const int c = e >> 4;
      const int wo = wo0 + pp;
      ra[q] = (wo < g.wo && co0 + c < g.co) ? dyn[((int64_t)(co0 + c) * g.ho + ho) * g.wo + wo] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) Bs[buf][bq * 8 + i][bcol] = rb[i];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 256 * q;
      As[buf][e & 15][e >> 4] = ra[q];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int lr = lane & 31, lk = lane >> 5;
  const int wn = wave * 32;
  load(0);
  store(0);
  __syncthreads();
  for (int it = 0; it < nsteps; ++it) {
    const int cur = it & 1;
    if (it + 1 < nsteps) load(it + 1);
#pragma unroll
    for (int kk = 0; kk < CBK; kk += 2) {
      const float a = As[cur][kk + lk][lr];
      const float b = Bs[cur][kk + lk][wn + lr];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    if (it + 1 < nsteps) store(cur ^ 1);
    __syncthreads();
  }
  const int col = kc0 + wn + lr;
  if (col < Kc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = co0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (c < g.co) partial[((int64_t)n * g.co + c) * Kc + col] = acc[r];
    }
  }
}

// dw[i] = sum_n partial[n][i]  (fixed order -> deterministic)
__global__ void wgrad_reduce_kernel(const float* __restrict__ partial, int N, int64_t per,
                                    float* __restrict__ dw) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per;
       i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
#pragma unroll 8
    for (int n = 0; n < N; ++n) s += partial[(int64_t)n * per + i];   // loads in flight, order kept
    dw[i] = s;
  }
}

// dbias[co] = sum over (n, ho, wo) of dy; one 1024-thread block per channel, eight loads
// in flight per thread (a channel is N planes: 5.2 MB for conv1), fp64 sums in a fixed order.
constexpr int BG_T = 1024;
__global__ __launch_bounds__(BG_T) void bias_grad_kernel(const float* __restrict__ dy, int N, int C,
                                                         int64_t plane, float* __restrict__ db) {
  const int c = blockIdx.x;
  double acc = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* p = dy + ((int64_t)n * C + c) * plane;
    int64_t i = threadIdx.x;
    for (; i + 7 * BG_T < plane; i += 8 * BG_T) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p[i + k * BG_T];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; i < plane; i += BG_T) acc += p[i];
  }
  __shared__ double red[BG_T / 64];
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < BG_T / 64; ++w) t += red[w];
    db[c] = static_cast<float>(t);
  }
}

// ---------------------------------------------------------------------------
// Direct convolution from an LDS input patch (width stride 1): forward and dgrad.
//
// A workgroup owns 32 output channels x PT_ROWS output rows x PT_COLS output
// columns of one sample; wave w computes row w with four 32x32 MFMA tiles.  For
// each input ("loop") channel the input patch those outputs need — rows
// PR0 + w*RSI + a, columns PC0 + j + b — and the channel's filter taps Wl[t][m]
// (t = a*B + b) are staged once in LDS; every tap is then one A read (weights),
// four B reads (patch, consecutive columns across lanes) and four MFMAs.  Versus
// the im2col gather this reads each input element from global memory once per
// workgroup instead of once per tap.  The next channel's patch and taps are
// loaded into registers while the current channel's MFMAs run.
//
//   fwd  : out = y[n][co][ho][wo], loop over ci, taps (kh, kw),
//          input row = ho*sh - ph + kh, col = wo - pw + kw
//   dgrad: out = dx[n][ci][hi][wi] for the rows hi of one stride class
//          (hi + ph) % sh == q; loop over co, taps = the kh of that class
//          (reversed) x the kw (reversed), input = dy row
//          (hi + ph - kh) / sh, col = wi + pw - kw
constexpr int PT_PREG = (PT_PROWS * (PT_PITCH - 6) + 255) / 256;
constexpr int PT_WREG4 = (PT_TMAX * PT_WP / 4 + 255) / 256;

struct PatchGeom {
  int taps_a;     // A: tap rows
  int tpad;       // A*B rounded up to even
  int prows;      // patch rows actually used (incl. the zero row)
  int pcols;      // patch columns actually used (PT_COLS + B - 1)
  int rsi;        // patch-row step between consecutive output rows of the tile
  int pr0;        // first patch row (input row index)
  int pc0;        // first patch column (input column index)
  int kh_class;   // dgrad: stride class q
  int r_first;    // first output row of the tile
  int r_step;     // output-row step between waves (1 fwd, sh dgrad)
};

template <bool DGRAD>
__device__ __forceinline__ PatchGeom patch_geom(const ConvDims& g, int ty, int wo0) {
  PatchGeom p;
  if (!DGRAD) {
    p.taps_a = g.kh;
    p.rsi = g.sh;
    p.r_first = ty * PT_ROWS;
    p.r_step = 1;
    p.pr0 = p.r_first * g.sh - g.ph;
    p.pc0 = wo0 - g.pw;
    p.kh_class = 0;
  } else {
    // decode (class q, tile) from ty: classes in order, ceil(count_q / PT_ROWS) tiles each
    int q = 0, t = ty, hq = 0;
    for (q = 0; q < g.sh; ++q) {
      const int cnt = class_rows(g, q, &hq);
      const int tiles = (cnt + PT_ROWS - 1) / PT_ROWS;
      if (t < tiles) break;
      t -= tiles;
    }
    const int aq = class_taps(g, q);
    p.taps_a = aq;
    p.rsi = 1;
    p.r_first = hq + g.sh * PT_ROWS * t;
    p.r_step = g.sh;
    p.pr0 = (p.r_first + g.ph - q) / g.sh - (aq - 1);
    p.pc0 = wo0 + g.pw - g.kw + 1;
    p.kh_class = q;
  }
  const int taps = p.taps_a * g.kw;
  p.tpad = (taps + 1) & ~1;
  p.prows = (PT_ROWS - 1) * p.rsi + p.taps_a + 1;
  p.pcols = PT_COLS + g.kw - 1;
  return p;
}

// Weight images, one [tstride][33] tile per (class, 32-channel output block, loop
// channel): img[t][m] = the weight of output channel m0+m for tap t (0 past the
// taps / channels).  fwd taps t = kh*kw + kw; dgrad taps of class q reversed.
template <bool DGRAD>
__global__ void conv_wimg_kernel(const float* __restrict__ w, ConvDims g, int tstride,
                                 float* __restrict__ img) {
  const int M = DGRAD ? g.ci : g.co;
  const int L = DGRAD ? g.co : g.ci;
  const int mbn = (M + 31) / 32;
  const int classes = DGRAD ? g.sh : 1;
  const int64_t tile = wimg_tile(tstride);
  const int64_t total = (int64_t)classes * mbn * L * tile;
  const int KHW = g.kh * g.kw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int e = static_cast<int>(r % tile); r /= tile;
    const int c = static_cast<int>(r % L); r /= L;
    const int mb = static_cast<int>(r % mbn); r /= mbn;
    const int q = static_cast<int>(r);
    const int t = e / PT_WP;
    const int m = mb * 32 + (e - t * PT_WP);
    float v = 0.f;
    if (t < tstride && e - t * PT_WP < 32 && m < M) {
      const int a = t / g.kw;
      const int b = t - a * g.kw;
      if (!DGRAD) {
        if (a < g.kh) v = w[((int64_t)m * g.ci + c) * KHW + a * g.kw + b];
      } else {
        const int aq = class_taps(g, q);
        if (a < aq) {
          const int khi = q + g.sh * (aq - 1 - a);
          v = w[((int64_t)c * g.ci + m) * KHW + khi * g.kw + (g.kw - 1 - b)];
        }
      }
    }
    img[i] = v;
  }
}

template <bool DGRAD>
__global__ __launch_bounds__(256) void conv_patch_kernel(const float* __restrict__ in,
                                                         const float* __restrict__ img,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ out, ConvDims g,
                                                         const int* __restrict__ out_lens,
                                                         int tstride, int gx, int gy) {
  __shared__ __attribute__((aligned(16))) float ps[PT_PROWS * PT_PITCH];
  __shared__ __attribute__((aligned(16))) float wl[PT_TMAX * PT_WP];
  const int M = DGRAD ? g.ci : g.co;            // output channels
  const int L = DGRAD ? g.co : g.ci;            // loop channels
  const int in_h = DGRAD ? g.ho : g.hi;
  const int in_w = DGRAD ? g.wo : g.wi;
  const int out_h = DGRAD ? g.hi : g.ho;
  const int out_w = DGRAD ? g.wi : g.wo;
  const int mbn = (M + 31) / 32;
  int bx, by, bz;
  xcd_tile(gx, gy, bx, by, bz);
  const int n = bz / mbn;
  const int mb = bz - n * mbn;
  const int m0 = mb * 32;
  const int c0 = bx * PT_COLS;
  const PatchGeom p = patch_geom<DGRAD>(g, by, c0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int B = g.kw;
  const int plane = in_h * in_w;
  const float* inn = in + (int64_t)n * L * plane;
  const int64_t tile = wimg_tile(tstride);
  const float* wimg = img + ((int64_t)p.kh_class * mbn + mb) * L * tile;
  const int wq = (p.tpad * PT_WP + 3) / 4;      // 16-byte chunks of the used tap rows
  const int pe = p.prows * p.pcols;

  // channel-invariant part of this thread's patch offsets: (row, col) of idx = tid + 256 r
  float rp[PT_PREG];
  u32x4 rw[PT_WREG4];
  auto load = [&](int c) {
    const __amdgpu_buffer_rsrc_t rs = conv_rsrc(inn + (int64_t)c * plane, plane);
    int row = tid / p.pcols, col = tid - (tid / p.pcols) * p.pcols;
#pragma unroll
    for (int r = 0; r < PT_PREG; ++r) {
      const int ir = p.pr0 + row, ic = p.pc0 + col;
      const bool ok = tid + 256 * r < pe && row < p.prows - 1 && ir >= 0 && ir < in_h &&
                      ic >= 0 && ic < in_w;
      rp[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                            rs, ok ? (ir * in_w + ic) * 4 : 0x7ffffff0, 0, 0));
      col += 256;
      while (col >= p.pcols) {
        col -= p.pcols;
        ++row;
      }
    }
    const __amdgpu_buffer_rsrc_t ws = conv_rsrc(wimg + (int64_t)c * tile, tile);
#pragma unroll
    for (int r = 0; r < PT_WREG4; ++r) {
      const int i = tid + 256 * r;
      rw[r] = __builtin_amdgcn_raw_buffer_load_b128(ws, i < wq ? i * 16 : 0x7ffffff0, 0, 0);
    }
  };
  auto store = [&]() {
    int row = tid / p.pcols, col = tid - (tid / p.pcols) * p.pcols;
#pragma unroll
    for (int r = 0; r < PT_PREG; ++r) {
      if (tid + 256 * r < pe) ps[row * PT_PITCH + col] = rp[r];
      col += 256;
      while (col >= p.pcols) {
        col -= p.pcols;
        ++row;
      }
    }
#pragma unroll
    for (int r = 0; r < PT_WREG4; ++r) {
      const int i = tid + 256 * r;
      if (i < wq) *reinterpret_cast<u32x4*>(wl + 4 * i) = rw[r];
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const int lr = lane & 31, lk = lane >> 5;
  // this lane's first tap (t = lk) as (a, b) and its patch offset
  const int a0 = lk / B, b0 = lk - (lk / B) * B;
  const int po_start = (wave * p.rsi + a0) * PT_PITCH + b0 + lr;
  const int steps = p.tpad >> 1;

  load(0);
  store();
  __syncthreads();
  for (int c = 0; c < L; ++c) {
    if (c + 1 < L) load(c + 1);
    int po = po_start, bb = b0;
    const float* wrow = wl + lk * PT_WP + lr;
    // Two operand sets in ping-pong: the reads of step s + 1 are issued before the MFMAs
    // of step s (sched barriers keep that order), so the LDS latency hides behind this
    // wave's own MFMAs.  A step past the end re-reads a valid address with A = 0.
    auto advance = [&]() {
      bb += 2;
      po += 2;
      if (bb >= B) {            // kw >= 2 (host-checked): at most one wrap per step
        bb -= B;
        po += PT_PITCH - B;
      }
    };
    auto read = [&](int st, float& av, float (&v)[4]) {
      const bool ok = st < steps;
      const float* pp = ps + (ok ? po : po_start);
      av = ok ? wrow[st * 2 * PT_WP] : 0.f;
      v[0] = pp[0]; v[1] = pp[32]; v[2] = pp[64]; v[3] = pp[96];
    };
    auto mma = [&](float av, const float (&v)[4]) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, v[j], acc[j], 0, 0, 0);
    };
    float aA, aB, vA[4], vB[4];
    read(0, aA, vA);
    // a wave whose output row lies past the plane (the last row tile of 41 / 81 rows)
    // skips its MFMAs: its SIMD time goes to the other workgroups' waves on the CU
    const int nsteps = p.r_first + wave * p.r_step < out_h ? steps : 0;
    for (int s = 0; s < nsteps; s += 2) {
      advance();
      read(s + 1, aB, vB);
      __builtin_amdgcn_sched_barrier(0);
      mma(aA, vA);
      __builtin_amdgcn_sched_barrier(0);
      advance();
      read(s + 2, aA, vA);
      __builtin_amdgcn_sched_barrier(0);
      mma(aB, vB);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if (c + 1 < L) {
      store();
      __syncthreads();
    }
  }

  const int orow = p.r_first + wave * p.r_step;
  if (orow >= out_h) return;
  const int len = (!DGRAD && out_lens != nullptr) ? out_lens[n] : out_w;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + 32 * j + lr;
    if (col >= out_w) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (m < M) {
        float v = acc[j][r];
        if (!DGRAD) {
          if (bias != nullptr) v += bias[m];
          if (col >= len) v = 0.f;
        }
        out[(((int64_t)n * M + m) * out_h + orow) * out_w + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Weight gradient from LDS tiles: for one (sample n, input channel ci, band of
// output rows) a workgroup accumulates
//   dW[co][ci][t] += sum_pos dy[n][co][pos] * x[n][ci][row(pos, kh)][col(pos, kw)]
// for all 32 co and all taps t = kh*kw + kw, as MFMA tiles with M = co, N = 32
// taps, K = output positions.  Per chunk of WG_RW x WG_CW output positions the
// dy tile (position-major, 33-float rows: conflict-free A reads) and the x patch
// those positions touch are staged once in LDS; a lane's tap is fixed, so every
// B read is the lane's tap offset plus the position offset.  Partials per
// (n, band) are reduced in a fixed order by wgrad_reduce_kernel (deterministic).
constexpr int WG_DYP = 33;          // dy tile row pitch

template <int NT, int XS, int SW>
__global__ __launch_bounds__(256) void conv_wgrad_patch_kernel(const float* __restrict__ dy,
                                                               const float* __restrict__ x,
                                                               float* __restrict__ partial,
                                                               ConvDims g, int bands, int xpitch) {
  int bx, by, bz;
  xcd_tile(bands, g.ci, bx, by, bz);
  __shared__ __attribute__((aligned(16))) float dys[WG_RW * WG_CW * WG_DYP];
  __shared__ __attribute__((aligned(16))) float xs[XS];
  constexpr int DYREG = WG_RW * WG_CW * 32 / 256;
  constexpr int XREG = (XS + 255) / 256;
  const int band = bx;
  const int ci = by;
  const int mbn = (g.co + 31) / 32;
  const int n = bz / mbn;
  const int m0 = (bz - n * mbn) * 32;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lr = lane & 31, lk = lane >> 5;
  const int T = g.kh * g.kw;
  const int Kc = g.ci * T;
  const int prow = (WG_RW - 1) * g.sh + g.kh;          // patch rows
  const int pcol = (WG_CW - 1) * g.sw + g.kw;          // patch columns
  const int pe = prow * pcol;
  // band = an equal share of the sample's (row chunk, column tile) list, so every
  // workgroup of a launch carries the same MFMA work (whole row-chunk bands left a third of
  // conv1's workgroups idle or in a half-empty second round)
  const int rchunks = (g.ho + WG_RW - 1) / WG_RW;
  const int ctiles = (g.wo + WG_CW - 1) / WG_CW;
  const int nck = rchunks * ctiles;
  const int kc0 = static_cast<int>((int64_t)band * nck / bands);
  const int nchunks = static_cast<int>((int64_t)(band + 1) * nck / bands) - kc0;
  const int dplane = g.ho * g.wo;
  const int xplane = g.hi * g.wi;
  const __amdgpu_buffer_rsrc_t drs =
      conv_rsrc(dy + ((int64_t)n * g.co + m0) * dplane, (int64_t)min(32, g.co - m0) * dplane);
  const __amdgpu_buffer_rsrc_t xrs = conv_rsrc(x + ((int64_t)n * g.ci + ci) * xplane, xplane);

  // this lane's taps (one per tile) as patch offsets; invalid taps read offset 0
  int tb[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int t = (wave * NT + j) * 32 + lr;
    tb[j] = t < T ? (t / g.kw) * xpitch + (t - (t / g.kw) * g.kw) : 0;
  }

  float rd[DYREG], rx[XREG];
  auto load = [&](int k) {
    const int kk = kc0 + k;
    const int rc = kk / ctiles;
    const int ho0 = rc * WG_RW;
    const int wo0 = (kk - rc * ctiles) * WG_CW;
#pragma unroll
    for (int r = 0; r < DYREG; ++r) {
      const int idx = tid + 256 * r;                  // (co, row, col), col fastest
      const int co = idx / (WG_RW * WG_CW);
      const int rr = (idx / WG_CW) % WG_RW;
      const int cc = idx % WG_CW;
      const int ho = ho0 + rr, wo = wo0 + cc;
      const bool ok = m0 + co < g.co && ho < g.ho && wo < g.wo;
      rd[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                            drs, ok ? (co * dplane + ho * g.wo + wo) * 4 : 0x7ffffff0, 0, 0));
    }
    const int ir0 = ho0 * g.sh - g.ph, ic0 = wo0 * g.sw - g.pw;
    int row = tid / pcol, col = tid - (tid / pcol) * pcol;
#pragma unroll
    for (int r = 0; r < XREG; ++r) {
      const int ir = ir0 + row, ic = ic0 + col;
      const bool ok = tid + 256 * r < pe && ir >= 0 && ir < g.hi && ic >= 0 && ic < g.wi;
      rx[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                            xrs, ok ? (ir * g.wi + ic) * 4 : 0x7ffffff0, 0, 0));
      col += 256;
      while (col >= pcol) {
        col -= pcol;
        ++row;
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int r = 0; r < DYREG; ++r) {
      const int idx = tid + 256 * r;
      const int co = idx / (WG_RW * WG_CW);
      const int pos = idx % (WG_RW * WG_CW);
      dys[pos * WG_DYP + co] = rd[r];
    }
    int row = tid / pcol, col = tid - (tid / pcol) * pcol;
#pragma unroll
    for (int r = 0; r < XREG; ++r) {
      if (tid + 256 * r < pe) xs[row * xpitch + col] = rx[r];
      col += 256;
      while (col >= pcol) {
        col -= pcol;
        ++row;
      }
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  if (nchunks > 0) {
    load(0);
    store();
  }
  __syncthreads();
  const int rstep = g.sh * xpitch;
  for (int k = 0; k < nchunks; ++k) {
    if (k + 1 < nchunks) load(k + 1);
    const float* arow = dys + lk * WG_DYP + lr;
    // per output row of the chunk one base per tap tile; the position pairs of the row are then
    // fixed offsets (width stride SW a template parameter): no per-position index arithmetic
    // (software-pipelining these reads a position pair ahead measured slower: 0.58 -> 0.66 ms)
#pragma unroll
    for (int rr = 0; rr < WG_RW; ++rr) {
      const float* ar = arow + rr * WG_CW * WG_DYP;
      const float* xb[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) xb[j] = xs + tb[j] + rr * rstep + lk * SW;
#pragma unroll 8
      for (int s = 0; s < WG_CW / 2; ++s) {
        const float av = ar[2 * s * WG_DYP];
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[j][2 * s * SW], acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
    if (k + 1 < nchunks) {
      store();
      __syncthreads();
    }
  }
  float* out = partial + ((int64_t)n * bands + band) * g.co * Kc;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int t = (wave * NT + j) * 32 + lr;
    if (t >= T) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (m < g.co) out[(int64_t)m * Kc + ci * T + t] = acc[j][r];
    }
  }
}

// ---------------------------------------------------------------------------
// Single-input-channel forward from an LDS patch (conv1: 1 -> 32 channels, 41 x 11 taps,
// stride 2 x 2) on v_mfma_f32_32x32x2_f32: M = 32 output channels, N = 32 output columns,
// K = taps.  A workgroup owns one sample's C1_RW output rows x C1_WC output columns; the
// input patch those outputs read (47 x 265 floats for conv1) and the whole filter bank as
// [tap][co] (452 x 32 floats) are staged in LDS once, then every k-pair is one A read (32
// consecutive channels), two B reads (patch offset of the lane's tap + its column * stride;
// consecutive taps differ by an odd offset, so the two half-waves hit disjoint banks) and two
// MFMAs.  The implicit-GEMM conv_fwd_kernel gathered every tap of every position from global
// memory instead (16 scattered loads + index arithmetic per thread per 16 taps).
// Wave w: output row w >> 1, columns (w & 1) * 64 + [0, 64) as two 32-column tiles.
constexpr int C1_PREG = (C1_PATCH + C1_T - 1) / C1_T;
constexpr int C1_WREG = (32 * C1_KROWS + C1_T - 1) / C1_T;
static_assert(2 * C1_PATCH * 4 + C1_KROWS * 32 * 4 <= 160 * 1024, "conv1 patch kernel LDS");

// KWH = kernel columns padded to even, halved (conv1: 11 -> 12 -> 6): a k-pair is two
// adjacent columns of one tap row, so every LDS read of the inner loop is a fixed offset
// from a per-row base (no per-tap index arithmetic: the stepped-tap form spent ~10 VALU per
// MFMA, SQ_INSTS_VALU / SQ_INSTS_MFMA); the padded column has zero weight (+9 % MFMAs)
template <int KWH>
__global__ __launch_bounds__(C1_T, 1) void conv1_patch_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    float* __restrict__ y, ConvDims g, const int* __restrict__ out_lens, int gx, int gy,
    int tiles) {
  // persistent: the filter bank is staged once per workgroup; the patch is double-buffered,
  // the next tile's loads in flight during this tile's MFMAs (one barrier per tile)
  constexpr int KW2 = 2 * KWH;
  __shared__ float ps[2][C1_PATCH];
  __shared__ float wsm[C1_KROWS * 32];
  const int T = g.kh * g.kw;
  const int PR = (C1_RW - 1) * g.sh + g.kh;
  const int PC = (C1_WC - 1) * g.sw + KW2;
  const int pe = PR * PC;
  // XCD-aware: the workgroups one XCD is dealt (ids congruent mod 8) take consecutive tiles
  // of every round (neighbouring row tiles share 31 of their 47 patch rows in that L2)
  const int G = gridDim.x;
  const int q8 = G >> 3, r8 = G & 7, xcd = blockIdx.x & 7;
  const int slot = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
  float rp[C1_PREG];
  const int r00 = threadIdx.x / PC, c00 = threadIdx.x - (threadIdx.x / PC) * PC;
  const int dr = C1_T / PC, dc = C1_T - (C1_T / PC) * PC;
  auto tile_of = [&](int t, int& n, int& ho0, int& wo0) {
    const int bx = t % gx, rest = t / gx;
    wo0 = bx * C1_WC;
    ho0 = (rest % gy) * C1_RW;
    n = rest / gy;
  };
  // every load of a patch issued before its LDS stores (indices stepped, no division)
  auto load_patch = [&](int t) {
    int n, ho0, wo0;
    tile_of(t, n, ho0, wo0);
    const int ir0 = ho0 * g.sh - g.ph, ic0 = wo0 * g.sw - g.pw;
    const float* xn = x + (int64_t)n * g.hi * g.wi;
    int r = r00, c = c00;
#pragma unroll
    for (int u = 0; u < C1_PREG; ++u) {
      const int ir = ir0 + r, ic = ic0 + c;
      const bool ok = threadIdx.x + u * C1_T < pe && ir >= 0 && ir < g.hi && ic >= 0 && ic < g.wi;
      rp[u] = ok ? xn[(int64_t)ir * g.wi + ic] : 0.f;
      r += dr;
      c += dc;
      if (c >= PC) {
        c -= PC;
        ++r;
      }
    }
  };
  auto store_patch = [&](float* dst) {
#pragma unroll
    for (int u = 0; u < C1_PREG; ++u)
      if (threadIdx.x + u * C1_T < pe) dst[threadIdx.x + u * C1_T] = rp[u];
  };
  int t = slot;
  if (t >= tiles) return;
  load_patch(t);
  {
    // the bank read in its own [co][tap] order (coalesced), stored as [tap row x kw2][co];
    // the padded column's rows are zero
    float rw[C1_WREG];
    int wk[C1_WREG];
    int co = threadIdx.x / T, k = threadIdx.x - (threadIdx.x / T) * T;
    const int dco = C1_T / T, dk = C1_T - (C1_T / T) * T;
#pragma unroll
    for (int u = 0; u < C1_WREG; ++u) {
      const bool in = co < 32;
      rw[u] = (in && co < g.co) ? w[(int64_t)co * T + k] : 0.f;
      const int a = k / g.kw;
      wk[u] = in ? ((a * KW2 + (k - a * g.kw)) << 5) + co : -1;
      co += dco;
      k += dk;
      if (k >= T) {
        k -= T;
        ++co;
      }
    }
    store_patch(ps[0]);
#pragma unroll
    for (int u = 0; u < C1_WREG; ++u)
      if (wk[u] >= 0) wsm[wk[u]] = rw[u];
    for (int j = threadIdx.x; j < g.kh * (KW2 - g.kw) * 32; j += C1_T) {
      const int a = (j >> 5) / (KW2 - g.kw), b = g.kw + (j >> 5) - a * (KW2 - g.kw);
      wsm[((a * KW2 + b) << 5) + (j & 31)] = 0.f;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lr = lane & 31, lk = lane >> 5;
  const int orow = wave >> 1;
  const int ocol = (wave & 1) * 64;
  // lane half lk takes kernel column 2p + lk of the pair
  const int poff = orow * g.sh * PC + (ocol + lr) * g.sw + lk;
  const float* wa = wsm + lk * 32 + lr;
  for (int cur = 0; t < tiles; t += G, cur ^= 1) {
    const bool more = t + G < tiles;
    if (more) load_patch(t + G);
    const float* pb0 = ps[cur] + poff;
    const float* pb1 = pb0 + 32 * g.sw;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc0[r] = 0.f;
      acc1[r] = 0.f;
    }
    for (int a = 0; a < g.kh; ++a) {
      const float* r0 = pb0 + a * PC;
      const float* r1 = pb1 + a * PC;
      const float* wr = wa + a * KW2 * 32;
#pragma unroll
      for (int p = 0; p < KWH; ++p) {
        const float av = wr[2 * p * 32];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, r0[2 * p], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, r1[2 * p], acc1, 0, 0, 0);
      }
    }
    // nobody reads the other buffer this round (the last barrier followed every wave's
    // previous round of reads): fill it, then one barrier before it is read
    if (more) store_patch(ps[cur ^ 1]);
    int n, ho0, wo0;
    tile_of(t, n, ho0, wo0);
    const int ho = ho0 + orow;
    if (ho < g.ho) {
      const int len = out_lens != nullptr ? out_lens[n] : g.wo;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = wo0 + ocol + 32 * j + lr;
        if (col >= g.wo) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (c < g.co) {
            float v = (j == 0 ? acc0[r] : acc1[r]) + (bias != nullptr ? bias[c] : 0.f);
            if (col >= len) v = 0.f;
            y[(((int64_t)n * g.co + c) * g.ho + ho) * g.wo + col] = v;
          }
        }
      }
    }
    __syncthreads();
  }
}


static int conv_cus() {
  static int cus = -1;
  if (cus < 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    cus = v;
  }
  return cus;
}

template <bool DGRAD>
static ds2_status_t launch_patch(const ConvPlan& p, const ConvDims& g, const float* in,
                                 const float* w, const float* bias, float* out,
                                 const int* out_lens, void* ws, hipStream_t st) {
  float* img = static_cast<float*>(ws);
  hipLaunchKernelGGL(conv_wimg_kernel<DGRAD>, dim3(std::min(cdiv(p.img, 256), 2048)), dim3(256), 0,
                     st, w, g, p.tstride, img);
  hipLaunchKernelGGL(conv_patch_kernel<DGRAD>, dim3(static_cast<unsigned>(p.grid)), dim3(256), 0, st,
                     in, img, bias, out, g, out_lens, p.tstride, p.gx, p.gy);
  return launch_status(DGRAD ? "ds2_conv2d_dgrad" : "ds2_conv2d_fwd");
}

// the caller's workspace covers the plan; the one-row grid fits a launch
static inline ds2_status_t plan_fits(const ConvPlan& p, const void* ws, size_t ws_bytes) {
  if (p.ws_bytes > 0 && (ws == nullptr || ws_bytes < p.ws_bytes)) return DS2_WORKSPACE_TOO_SMALL;
  return p.too_big ? DS2_UNSUPPORTED_SHAPE : DS2_OK;
}

}  // namespace ds2

using namespace ds2;

extern "C" {

size_t ds2_conv2d_workspace_size(int n, int c_in, int h_in, int w_in, int c_out, int kh, int kw,
                                 int sh, int sw, int ph, int pw) {
  ConvDims g;
  if (!make_dims(g, n, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw)) return 0;
  return conv_ws_max(g, conv_switches());
}

ds2_status_t ds2_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int n,
                            int c_in, int h_in, int w_in, int c_out, int kh, int kw, int sh,
                            int sw, int ph, int pw, const int* out_lens, void* ws,
                            size_t ws_bytes, ds2_stream_t stream) {
  ConvDims g;
  if (!make_dims(g, n, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw)) return DS2_INVALID_VALUE;
  if (n == 0) return DS2_OK;
  if (g.ho > 65535) return DS2_UNSUPPORTED_SHAPE;
  const ConvPlan p = conv_plan_fwd(g, conv_switches());
  const ds2_status_t fits = plan_fits(p, ws, ws_bytes);
  if (fits != DS2_OK) return fits;
  hipStream_t st = as_stream(stream);
  switch (p.rung) {
    case DS2_CONV_FWD_PATCH:
      return launch_patch<false>(p, g, x, w, bias, y, out_lens, ws, st);
    case DS2_CONV_FWD_C1: {
      const int grid = static_cast<int>(std::min<int64_t>(p.grid, conv_cus()));   // one per CU
      const auto k = p.a == 6 ? conv1_patch_fwd_kernel<6> : p.a == 5 ? conv1_patch_fwd_kernel<5>
                   : p.a == 4 ? conv1_patch_fwd_kernel<4> : p.a == 3 ? conv1_patch_fwd_kernel<3>
                                                                      : conv1_patch_fwd_kernel<2>;
      hipLaunchKernelGGL(k, dim3(grid), dim3(C1_T), 0, st, x, w, bias, y, g, out_lens, p.gx, p.gy,
                         static_cast<int>(p.grid));
      return launch_status("ds2_conv2d_fwd");
    }
    case DS2_CONV_FWD_GEMM: {
      dim3 grid(cdiv(g.wo, CBN), g.ho, n * cdiv(c_out, 32));
      hipLaunchKernelGGL(conv_fwd_kernel, grid, dim3(256), 0, st, x, w, bias, y, g, out_lens);
      return launch_status("ds2_conv2d_fwd");
    }
    default:
      return launch_conv_split(p, g, x, w, bias, y, out_lens, ws, st);
  }
}

ds2_status_t ds2_conv2d_dgrad(const float* dy, const float* w, float* dx, int n, int c_in,
                              int h_in, int w_in, int c_out, int kh, int kw, int sh, int sw,
                              int ph, int pw, void* ws, size_t ws_bytes, ds2_stream_t stream) {
  ConvDims g;
  if (!make_dims(g, n, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw)) return DS2_INVALID_VALUE;
  if (n == 0) return DS2_OK;
  const ConvPlan p = conv_plan_dgrad(g, conv_switches());
  const ds2_status_t fits = plan_fits(p, ws, ws_bytes);
  if (fits != DS2_OK) return fits;
  hipStream_t st = as_stream(stream);
  switch (p.rung) {
    case DS2_CONV_DG_PATCH:
      return launch_patch<true>(p, g, dy, w, nullptr, dx, nullptr, ws, st);
    case DS2_CONV_DG_GEMM: {
      dim3 grid(cdiv(w_in, CBN), h_in, n * cdiv(c_in, 32));
      hipLaunchKernelGGL(conv_dgrad_kernel, grid, dim3(256), 0, st, dy, w, dx, g);
      return launch_status("ds2_conv2d_dgrad");
    }
    default:
      return launch_conv_split(p, g, dy, w, nullptr, dx, nullptr, ws, st);
  }
}

size_t ds2_conv2d_wgrad_workspace_size(int n, int c_in, int h_in, int w_in, int c_out, int kh,
                                       int kw, int sh, int sw, int ph, int pw) {
  ConvDims g;
  if (!make_dims(g, n, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw)) return 0;
  return conv_plan_wgrad(g, conv_switches()).ws_bytes;
}

ds2_status_t ds2_conv2d_wgrad(const float* dy, const float* x, float* dw, float* dbias, int n,
                              int c_in, int h_in, int w_in, int c_out, int kh, int kw, int sh,
                              int sw, int ph, int pw, void* ws, size_t ws_bytes,
                              ds2_stream_t stream) {
  ConvDims g;
  if (!make_dims(g, n, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw)) return DS2_INVALID_VALUE;
  if (n == 0) return DS2_OK;
  const ConvPlan p = conv_plan_wgrad(g, conv_switches());
  if (ws == nullptr || ws_bytes < p.ws_bytes) return DS2_WORKSPACE_TOO_SMALL;
  hipStream_t st = as_stream(stream);
  float* partial = static_cast<float*>(ws);
  const int64_t per = (int64_t)c_out * c_in * kh * kw;
  int slabs = n;
  switch (p.rung) {
    case DS2_CONV_WG_PATCH: {
      const auto k = p.a == 2 ? (p.b == 2 ? conv_wgrad_patch_kernel<2, WG_XS_SMALL, 2>
                                          : conv_wgrad_patch_kernel<2, WG_XS_SMALL, 1>)
                              : (p.b == 2 ? conv_wgrad_patch_kernel<4, WG_XS_LARGE, 2>
                                          : conv_wgrad_patch_kernel<4, WG_XS_LARGE, 1>);
      hipLaunchKernelGGL(k, dim3(static_cast<unsigned>(p.grid)), dim3(256), 0, st, dy, x, partial, g,
                         p.bands, p.pitch);
      slabs = n * p.bands;
      break;
    }
    case DS2_CONV_WG_GEMM: {
      dim3 grid(cdiv(c_in * kh * kw, CBNW), n, cdiv(c_out, 32));
      hipLaunchKernelGGL(conv_wgrad_kernel, grid, dim3(256), 0, st, dy, x, partial, g);
      break;
    }
    default: {
      const ds2_status_t rc = launch_conv_split_wgrad(p, g, dy, x, dw, ws, st);
      if (rc != DS2_OK) return rc;
      slabs = 0;   // reduced there
    }
  }
  if (slabs > 0)
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(std::min(cdiv(per, 256), 2048)), dim3(256), 0, st,
                       partial, slabs, per, dw);
  if (dbias != nullptr)
    hipLaunchKernelGGL(bias_grad_kernel, dim3(c_out), dim3(BG_T), 0, st, dy, n, c_out,
                       (int64_t)g.ho * g.wo, dbias);
  return launch_status("ds2_conv2d_wgrad");
}

ds2_status_t ds2_test_conv2d_plan(int dir, int n, int c_in, int h_in, int w_in, int c_out, int kh,
                                  int kw, int sh, int sw, int ph, int pw, int* out) {
  ConvDims g;
  if (dir < 0 || dir > 2 || out == nullptr ||
      !make_dims(g, n, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw))
    return DS2_INVALID_VALUE;
  const ConvSwitches s = conv_switches();
  const ConvPlan p = dir == 0 ? conv_plan_fwd(g, s) : dir == 1 ? conv_plan_dgrad(g, s)
                                                               : conv_plan_wgrad(g, s);
  const int vals[11] = {p.rung, p.a, p.b,
                        static_cast<int>(p.ws_bytes & 0xffffffffu),
                        static_cast<int>((uint64_t)p.ws_bytes >> 32),
                        p.gx, p.gy, p.splits, p.bands, p.pitch,
                        static_cast<int>(std::min<int64_t>(p.grid, 0x7fffffff))};
  std::copy(vals, vals + 11, out);
  return DS2_OK;
}

}  // extern "C"
