// Conv1d (nn.Conv1d semantics, dilation 1, groups 1) on time-major activations, and the
// pointwise kernels of the Wav2Letter blocks (GLU, BatchNorm + ReLU).
//
//   x [T][N][Cin] -> y [T_out][N][Cout],  T_out = (T + 2p - k) / s + 1,  w [Cout][Cin][k]
//
// Fast path: an implicit GEMM on v_mfma_f32_16x16x32_f16 at fp32-class accuracy (fp16x3, the
// two-term fp16 split under power-of-two row scales of gemm.hip's fp16x3 kernel; h3_exp /
// h3_scale in split_mma.h).  Output row (t, n) reads the window of k input rows t s - p ..
// t s - p + k - 1 of sample n, each a contiguous Cin run, so K = k Cin walks (tap, channel
// chunk of 32) stages; a tap outside [0, T) and the channels past Cin are predicated to zero
// in the loader (no padded copy of the activations).  The weights are re-laid once per call
// into the workspace as [Cout][k][Cin padded to 32] (forward) or, taps reversed,
// [Cin][k][Cout padded] (stride-1 dgrad = the same kernel on dy with padding k - 1 - p).
// The row scale of a window is the maximum of its rows' maxima (an upper bound is valid).
// wgrad is the transposed product: M = Cout, N = (tap, Cin), K = the T_out N output rows,
// both operands row-contiguous, split over K into slabs that a second kernel sums in a
// fixed order while it writes torch's [Cout][Cin][k] layout.
//
// General path (DS2_CONV1D=0, or a shape the fast path declines): an LDS-tiled fp32 FMA
// implicit GEMM over the same index maps, any stride / kernel / channel count.
// k = 1, s = 1, p = 0 is a plain GEMM and goes to ds2_sgemm_ws.
#include <stdlib.h>

#include "amax_rc.h"
#include "split_mma.h"

namespace ds2 {
namespace {

struct C1Dims {
  int t_in, n, ci, co, k, s, p, t_out;
};

bool fast_enabled() {
  const char* e = getenv("DS2_CONV1D");
  return !(e != nullptr && e[0] == '0');
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned ew_grid(int64_t total) {   // grid of a grid-stride elementwise kernel
  const int64_t g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
inline int pad32(int c) { return (c + 31) & ~31; }

// ---------------------------------------------------------------------------
// operand maxima (float bits; non-negative floats order as unsigned)
__global__ __launch_bounds__(256) void c1_rowmax_kernel(const float* __restrict__ x, int rows,
                                                        int cols, unsigned* __restrict__ out) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* xr = x + (int64_t)r * cols;
  float m = 0.f;
  for (int c = lane; c < cols; c += 64) m = fmaxf(m, fabsf(xr[c]));
  m = wave_max(m);
  if (lane == 0) out[r] = __float_as_uint(m);
}

// out zeroed first; a block takes 128 rows, a thread the columns t, t + 256, ...
__global__ __launch_bounds__(256) void c1_colmax_kernel(const float* __restrict__ x, int rows,
                                                        int cols, unsigned* __restrict__ out) {
  const int r0 = blockIdx.x * 128, r1 = min(rows, r0 + 128);
  for (int c = threadIdx.x; c < cols; c += 256) {
    float m = 0.f;
    for (int r = r0; r < r1; ++r) m = fmaxf(m, fabsf(x[(int64_t)r * cols + c]));
    if (m > 0.f) atomicMax(out + c, __float_as_uint(m));
  }
}

// out [rows_o][k][qp]: flip == 0: rows_o = Cout, q = Cin: out[co][j][c] = w[co][c][j];
// flip == 1: rows_o = Cin, q = Cout: out[c][j][co] = w[co][c][k - 1 - j]; q >= its extent: 0
__global__ __launch_bounds__(256) void c1_relayout_w_kernel(const float* __restrict__ w, int co,
                                                            int ci, int k, int qp, int flip,
                                                            float* __restrict__ out) {
  const int rows_o = flip ? ci : co, qn = flip ? co : ci;
  const int64_t total = (int64_t)rows_o * k * qp;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % qp);
    const int j = (int)((i / qp) % k);
    const int r = (int)(i / ((int64_t)qp * k));
    float v = 0.f;
    if (q < qn) {
      const int o = flip ? q : r, c = flip ? r : q, js = flip ? k - 1 - j : j;
      v = w[((int64_t)o * ci + c) * k + js];
    }
    out[i] = v;
  }
}

// ---------------------------------------------------------------------------
// fp16x3 staging: LDS planes [rows][32 k] of fp16 (64-B rows), 16-B slot s of row r at
// s ^ ((r >> 1) & 3) (gemm.hip's layout for the 16x16x32 fragments: conflict-free reads)
constexpr int CK = 32;            // k per stage
constexpr int CT = 128;           // tile edge (rows of A and of B)
constexpr int CP = CT * CK;       // fp16 per plane
__device__ __forceinline__ int cslot(int row, int s) { return row * CK + 8 * (s ^ ((row >> 1) & 3)); }

// one stage of MFMAs: wave tile 64 x 64 = 4 x 4 tiles of 16 x 16, three products per pair
// (lo.hi + hi.lo + hi.hi; lo.lo, below 2^-22 |a b|, dropped)
__device__ __forceinline__ void c1_mma_stage(const unsigned short* __restrict__ as,
                                             const unsigned short* __restrict__ bs, int wm, int wn,
                                             int lane, f32x4 (&acc)[4][4]) {
  const int r16 = lane & 15, s16 = lane >> 4;
  f16x8 af[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int at = cslot(wm + 16 * i + r16, s16);
#pragma unroll
    for (int p = 0; p < 2; ++p) af[i][p] = *reinterpret_cast<const f16x8*>(as + p * CP + at);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f16x8 bq[2];
    const int bt = cslot(wn + 16 * j + r16, s16);
#pragma unroll
    for (int p = 0; p < 2; ++p) bq[p] = *reinterpret_cast<const f16x8*>(bs + p * CP + bt);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i][j] = mma3h(af[i][0], af[i][1], bq[0], bq[1], acc[i][j]);
    }
  }
}

// Two-level accumulation: the MFMAs of CFLUSH stages (256 k) sum into `acc`, which then joins
// `tot` and restarts from zero.  One fp32 chain over all of K (248 stages at K = 7936) walks
// its rounding error up with every stage; sums of 8 and then of K / 256 keep it at the level
// of a blocked fp32 sum.
constexpr int CFLUSH = 8;
__device__ __forceinline__ void c1_flush(f32x4 (&acc)[4][4], f32x4 (&tot)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tot[i][j] += acc[i][j];
      acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---------------------------------------------------------------------------
// Forward (and stride-1 dgrad on the flipped weights).  A: the activations x [t_in][n][ci],
// gathered; B: wr [co][k][cip] (cip = ci padded to 32, zeros past ci).  Stage kt = (tap j,
// channel chunk c0): a thread stages two (row, 8-k slot) units of A and of B, 256 threads,
// tile 128 x 128, two LDS stages, one barrier per stage; the next stage's global loads are
// in flight while this stage's MFMAs run.
template <bool VEC>
__global__ __launch_bounds__(256, 2) void c1_igemm_kernel(
    const float* __restrict__ x, const float* __restrict__ wr, const float* __restrict__ bias,
    float* __restrict__ y, const unsigned* __restrict__ x_rmax, const unsigned* __restrict__ w_rmax,
    C1Dims d, int cip) {
  __shared__ __attribute__((aligned(16))) unsigned short As[2][2 * CP];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[2][2 * CP];
  __shared__ int ea[CT], eb[CT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int n0 = blockIdx.x * CT;
  const int64_t m0 = (int64_t)blockIdx.y * CT;
  const int64_t M = (int64_t)d.t_out * d.n;

  // the exponents of the tile's rows (a window: the max over its valid taps) and columns
  if (t < CT) {
    const int64_t m = m0 + t;
    unsigned am = 0u;
    if (m < M) {
      const int to = (int)(m / d.n), nb = (int)(m - (int64_t)to * d.n);
      for (int j = 0; j < d.k; ++j) {
        const int ti = to * d.s - d.p + j;
        if (ti >= 0 && ti < d.t_in) am = max(am, x_rmax[(int64_t)ti * d.n + nb]);
      }
    }
    ea[t] = h3_exp(am);
  } else {
    const int c = n0 + t - CT;
    eb[t - CT] = c < d.co ? h3_exp(w_rmax[c]) : 0;
  }
  __syncthreads();

  // this thread's staging units: rows t >> 2 and 64 + (t >> 2), slot t & 3
  const int slot = t & 3;
  int a_ti0[2], a_nb[2];
  bool a_in[2], b_in[2];
  float a_sc[2], b_sc[2];
  const float* b_ptr[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = (t >> 2) + 64 * u;
    const int64_t m = m0 + row;
    a_in[u] = m < M;
    const int to = a_in[u] ? (int)(m / d.n) : 0;
    a_nb[u] = a_in[u] ? (int)(m - (int64_t)to * d.n) : 0;
    a_ti0[u] = to * d.s - d.p;
    a_sc[u] = h3_scale(ea[row]);
    const int c = n0 + row;
    b_in[u] = c < d.co;
    b_ptr[u] = wr + (int64_t)(b_in[u] ? c : 0) * d.k * cip + 8 * slot;
    b_sc[u] = h3_scale(eb[row]);
  }

  const int cpt = cip / CK;             // stages per tap
  const int stages = d.k * cpt;
  float ra[2][8], rb[2][8];
  auto load = [&](int kt) {
    const int j = kt / cpt, c0 = (kt - j * cpt) * CK + 8 * slot;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int ti = a_ti0[u] + j;
      const bool ok = a_in[u] && ti >= 0 && ti < d.t_in;
      const float* src = x + ((int64_t)(ok ? ti : 0) * d.n + a_nb[u]) * d.ci + c0;
      if (VEC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool in = ok && c0 + 4 * h < d.ci;        // ci % 4 == 0: whole float4 or none
          const f32x4 v = in ? *reinterpret_cast<const f32x4*>(src + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) ra[u][4 * h + e] = v[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) ra[u][e] = (ok && c0 + e < d.ci) ? src[e] : 0.f;
      }
      const float* bsrc = b_ptr[u] + (int64_t)kt * CK;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 v = b_in[u] ? *reinterpret_cast<const f32x4*>(bsrc + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[u][4 * h + e] = v[e];
      }
    }
  };

  f32x4 acc[4][4], tot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load(0);
  for (int kt = 0; kt < stages; ++kt) {
    const int cur = kt & 1;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int at = cslot((t >> 2) + 64 * u, slot);
      split_store8<2>(As[cur], CP, at, ra[u], a_sc[u]);
      split_store8<2>(Bs[cur], CP, at, rb[u], b_sc[u]);
    }
    // stage kt visible; the other buffer (stage kt - 1) is free once every wave is here
    __syncthreads();
    if (kt + 1 < stages) load(kt + 1);
    c1_mma_stage(As[cur], Bs[cur], wm, wn, lane, acc);
    if ((kt & (CFLUSH - 1)) == CFLUSH - 1) c1_flush(acc, tot);
  }
  c1_flush(acc, tot);

  // 16x16 C/D map: col = lane & 15, row = 4 (lane >> 4) + r; undo the scales (exact)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cl = wn + 16 * j + (lane & 15);
      const int col = n0 + cl;
      if (col >= d.co) continue;
      const float bv = bias != nullptr ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wm + 16 * i + 4 * (lane >> 4) + r;
        const int64_t row = m0 + rl;
        if (row < M) y[row * d.co + col] = __builtin_ldexpf(tot[i][j][r], -(ea[rl] + eb[cl])) + bv;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad: part[z][co][j ci + c] = sum over output rows r = (to, nb) of slab z of
// dy[r][co] x[(to s - p + j) n + nb][c].  Both operands are contiguous along their tile rows
// (co / c), so thread (row t & 127, k half t >> 7) loads 16 consecutive r for its row: each
// load instruction reads 64 consecutive floats of one activation row.
__global__ __launch_bounds__(256, 2) void c1_wgrad_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ part,
    const unsigned* __restrict__ dy_cmax, const unsigned* __restrict__ x_cmax, C1Dims d,
    int kchunk) {
  __shared__ __attribute__((aligned(16))) unsigned short As[2][2 * CP];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[2][2 * CP];
  __shared__ int ea[CT], eb[CT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int n0 = blockIdx.x * CT, m0 = blockIdx.y * CT;
  const int NN = d.k * d.ci;
  const int R = d.t_out * d.n;
  const int kbeg = blockIdx.z * kchunk, kend = min(R, kbeg + kchunk);

  if (t < CT) {
    const int co = m0 + t;
    ea[t] = co < d.co ? h3_exp(dy_cmax[co]) : 0;
  } else {
    const int nn = n0 + t - CT;
    eb[t - CT] = nn < NN ? h3_exp(x_cmax[nn % d.ci]) : 0;
  }
  __syncthreads();

  const int row = t & 127, kh = __builtin_amdgcn_readfirstlane(t >> 7);
  const int co = m0 + row, nn = n0 + row;
  const bool a_in = co < d.co, b_in = nn < NN;
  const int bj = b_in ? nn / d.ci : 0, bc = b_in ? nn - bj * d.ci : 0;
  const float a_sc = h3_scale(ea[row]), b_sc = h3_scale(eb[row]);

  float ra[16], rb[16];
  auto load = [&](int kt) {
    const int r0 = kbeg + kt * CK + 16 * kh;          // wave-uniform
    int to = r0 / d.n, nb = r0 - to * d.n;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = r0 + e;
      const bool rin = r < kend;
      ra[e] = (rin && a_in) ? dy[(int64_t)r * d.co + co] : 0.f;
      const int ti = to * d.s - d.p + bj;
      const bool ok = rin && b_in && ti >= 0 && ti < d.t_in;
      rb[e] = ok ? x[((int64_t)ti * d.n + nb) * d.ci + bc] : 0.f;
      if (++nb == d.n) {
        nb = 0;
        ++to;
      }
    }
  };

  f32x4 acc[4][4], tot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int stages = (kend - kbeg + CK - 1) / CK;
  if (stages > 0) load(0);
  for (int kt = 0; kt < stages; ++kt) {
    const int cur = kt & 1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int at = cslot(row, 2 * kh + h);
      split_store8<2>(As[cur], CP, at, ra + 8 * h, a_sc);
      split_store8<2>(Bs[cur], CP, at, rb + 8 * h, b_sc);
    }
    __syncthreads();
    if (kt + 1 < stages) load(kt + 1);
    c1_mma_stage(As[cur], Bs[cur], wm, wn, lane, acc);
    if ((kt & (CFLUSH - 1)) == CFLUSH - 1) c1_flush(acc, tot);
  }
  c1_flush(acc, tot);

  float* const pz = part + (int64_t)blockIdx.z * d.co * NN;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cl = wn + 16 * j + (lane & 15);
      const int col = n0 + cl;
      if (col >= NN) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wm + 16 * i + 4 * (lane >> 4) + r;
        const int rw = m0 + rl;
        if (rw < d.co) pz[(int64_t)rw * NN + col] = __builtin_ldexpf(tot[i][j][r], -(ea[rl] + eb[cl]));
      }
    }
  }
}

// dw[co][c][j] = sum over slabs z (ascending: deterministic) of part[z][co][j ci + c]
__global__ __launch_bounds__(256) void c1_wgrad_reduce_kernel(const float* __restrict__ part,
                                                              int nsplit, int co, int ci, int k,
                                                              float* __restrict__ dw) {
  const int64_t total = (int64_t)co * ci * k;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % k);
    const int c = (int)((i / k) % ci);
    const int o = (int)(i / ((int64_t)k * ci));
    const float* p = part + ((int64_t)o * k + j) * ci + c;
    float s = 0.f;
    for (int z = 0; z < nsplit; ++z) s += p[(int64_t)z * total];
    dw[i] = s;
  }
}

// ---------------------------------------------------------------------------
// General path: C[m][nn] = sum_kk A(m, kk) B(nn, kk) in fp32 FMA, tile 64 x 64 x 16, 256
// threads of 4 x 4 outputs; every stage's 16 products are summed on their own before they
// join the accumulator (shorter rounding chains than one serial sum over K).
//   MODE 0 forward: m = (to, nb), nn = co, kk = (j, c)
//   MODE 1 dgrad:   m = (ti, nb), nn = c,  kk = (j, co): to = (ti + p - j) / s where it divides
//   MODE 2 wgrad:   m = co, nn = (c, j) (torch's layout), kk = output row (to, nb)
template <int MODE>
__device__ __forceinline__ float c1_gen_a(const float* __restrict__ a, const C1Dims& d, int64_t m,
                                          int64_t kk) {
  if (MODE == 0) {
    const int j = (int)(kk / d.ci), c = (int)(kk - (int64_t)j * d.ci);
    const int to = (int)(m / d.n), nb = (int)(m - (int64_t)to * d.n);
    const int ti = to * d.s - d.p + j;
    return (ti >= 0 && ti < d.t_in) ? a[((int64_t)ti * d.n + nb) * d.ci + c] : 0.f;
  } else if (MODE == 1) {
    const int j = (int)(kk / d.co), o = (int)(kk - (int64_t)j * d.co);
    const int ti = (int)(m / d.n), nb = (int)(m - (int64_t)ti * d.n);
    const int num = ti + d.p - j;
    if (num < 0 || num % d.s != 0) return 0.f;
    const int to = num / d.s;
    return to < d.t_out ? a[((int64_t)to * d.n + nb) * d.co + o] : 0.f;
  } else {
    return a[kk * d.co + m];
  }
}
template <int MODE>
__device__ __forceinline__ float c1_gen_b(const float* __restrict__ b, const C1Dims& d, int64_t nn,
                                          int64_t kk) {
  if (MODE == 0) {
    const int j = (int)(kk / d.ci), c = (int)(kk - (int64_t)j * d.ci);
    return b[(nn * d.ci + c) * d.k + j];
  } else if (MODE == 1) {
    const int j = (int)(kk / d.co), o = (int)(kk - (int64_t)j * d.co);
    return b[((int64_t)o * d.ci + nn) * d.k + j];
  } else {
    const int c = (int)(nn / d.k), j = (int)(nn - (int64_t)c * d.k);
    const int to = (int)(kk / d.n), nb = (int)(kk - (int64_t)to * d.n);
    const int ti = to * d.s - d.p + j;
    return (ti >= 0 && ti < d.t_in) ? b[((int64_t)ti * d.n + nb) * d.ci + c] : 0.f;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void c1_general_kernel(const float* __restrict__ a,
                                                         const float* __restrict__ b,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ c, C1Dims d, int64_t M,
                                                         int64_t NN, int64_t K) {
  __shared__ float As[16][65], Bs[16][65];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int64_t m0 = (int64_t)blockIdx.y * 64, n0 = (int64_t)blockIdx.x * 64;
  float acc[4][4] = {};
  for (int64_t k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int id = t + 256 * e;
      // MODE 2: the operands are contiguous along m / nn; else along kk
      const int kk = MODE == 2 ? id >> 6 : id & 15, r = MODE == 2 ? id & 63 : id >> 4;
      const bool kin = k0 + kk < K;
      As[kk][r] = (kin && m0 + r < M) ? c1_gen_a<MODE>(a, d, m0 + r, k0 + kk) : 0.f;
      Bs[kk][r] = (kin && n0 + r < NN) ? c1_gen_b<MODE>(b, d, n0 + r, k0 + kk) : 0.f;
    }
    __syncthreads();
    float st[4][4] = {};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = As[kk][ty * 4 + i];
        bv[i] = Bs[kk][tx * 4 + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) st[i][j] = fmaf(av[i], bv[j], st[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += st[i][j];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + ty * 4 + i;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t nn = n0 + tx * 4 + j;
      if (nn < NN) c[m * NN + nn] = acc[i][j] + (bias != nullptr ? bias[nn] : 0.f);
    }
  }
}

// ---------------------------------------------------------------------------
// host side
bool dims_ok(int t, int n, int ci, int co, int k, int s, int p) {
  return t >= 0 && n >= 0 && ci >= 1 && co >= 1 && k >= 1 && s >= 1 && p >= 0;
}
int out_len(int t, int k, int s, int p) {
  const int num = t + 2 * p - k;
  return num < 0 ? 0 : num / s + 1;
}
bool fits_int(int64_t v) { return v < (1ll << 31); }

bool is_gemm(int k, int s, int p) { return k == 1 && s == 1 && p == 0; }
// the shapes the implicit GEMM takes (narrow layers would stage mostly padding)
bool fast_fwd(int ci, int co, int k) { return ci >= 16 && co >= 16 && (int64_t)k * ci >= 64; }
bool fast_dgrad(int ci, int co, int k, int s, int p) {
  return s == 1 && p <= k - 1 && fast_fwd(co, ci, k);
}
bool fast_wgrad(int ci, int co) { return ci >= 16 && co >= 16; }

// slabs of the wgrad's K = T_out N so that about two waves of workgroups cover the chip
int wgrad_split(int ci, int co, int k, int64_t rows, int* kchunk) {
  const int64_t tiles = (int64_t)cdiv((int64_t)k * ci, CT) * cdiv(co, CT);
  int64_t ns = (512 + tiles - 1) / tiles;
  const int64_t most = (rows + 255) / 256;        // at least 256 rows per slab
  if (ns > most) ns = most;
  if (ns < 1) ns = 1;
  int64_t ch = (rows + ns - 1) / ns;
  ch = (ch + CK - 1) / CK * CK;
  if (ch < CK) ch = CK;
  *kchunk = (int)ch;
  return (int)((rows + ch - 1) / ch);
}

size_t fwd_ws_fast(int t, int n, int ci, int co, int k, int t_out) {
  const int64_t wrf = (int64_t)co * k * pad32(ci), wdf = (int64_t)ci * k * pad32(co);
  const int tm = t > t_out ? t : t_out;
  return al256((size_t)(wrf > wdf ? wrf : wdf) * 4) + al256((size_t)tm * n * 4) +
         al256((size_t)(co > ci ? co : ci) * 4);
}

// the head of the wgrad workspace: ds2_colsum's (dbias) or, k = 1, ds2_sgemm_ws's
size_t wgrad_ws_head(int ci, int co, int k, int s, int p, int64_t rows) {
  size_t head = ds2_colsum_workspace_size((int)rows, co);
  if (is_gemm(k, s, p)) {
    const size_t g = ds2_sgemm_workspace_size(co, ci, (int)rows, 1);
    if (g > head) head = g;
  }
  return head;
}
size_t wgrad_ws(int ci, int co, int k, int s, int p, int64_t rows) {
  int kchunk = 0;
  const int ns = wgrad_split(ci, co, k, rows, &kchunk);
  return al256(wgrad_ws_head(ci, co, k, s, p, rows)) + al256((size_t)ci * 4) +
         al256((size_t)co * 4) + al256((size_t)ns * co * ci * k * 4) + 256;
}

// What one call launches: the one place that chooses.  The entry points (and the test hook
// ds2_test_conv1d_plan) switch on it; the values of `path` are the DS2_C1_* of ds2hip_test.h.
struct C1Plan {
  ds2_status_t status;   // != DS2_OK: returned before anything else is looked at
  int path;              // DS2_C1_NONE with DS2_OK: an empty call
  C1Dims d;              // the convolution the kernel computes (dgrad on the implicit GEMM: the
                         // forward of dy on the flipped weights, ci / co swapped, p = k - 1 - p)
  int stages;            // implicit GEMM: k pad32(d.ci) / 32
  unsigned gx, gy, gz;   // grid of the convolution kernel (GEMM: ds2_sgemm_ws's own plan, 0)
  int nsplit, kchunk;    // wgrad slabs
  size_t ws_bytes;       // checked before anything is launched; 0: NULL is taken
  int amax_passes;       // c1_rowmax_kernel / c1_colmax_kernel launches
};

// dir 0 forward, 1 dgrad, 2 wgrad; x_addr: the address of the gathered activations (forward: x,
// dgrad: dy), which decides the float4 loader; amax_given: the caller supplies their maxima
C1Plan c1_plan(int dir, int t, int n, int ci, int co, int k, int s, int p, uintptr_t x_addr,
               bool amax_given) {
  C1Plan pl{};
  pl.path = DS2_C1_NONE;
  pl.status = DS2_INVALID_VALUE;
  if (!dims_ok(t, n, ci, co, k, s, p)) return pl;
  const bool empty = t == 0 || n == 0;
  if (dir != 2 && empty) {
    pl.status = DS2_OK;
    return pl;
  }
  if (t + 2 * p - k < 0 && !empty) return pl;
  const int to = empty ? 0 : out_len(t, k, s, p);
  const int64_t rows = (int64_t)to * n;
  pl.status = DS2_UNSUPPORTED_SHAPE;
  if (!fits_int((int64_t)co * ci * k)) return pl;
  if (dir == 2 ? !fits_int(rows) : !fits_int((int64_t)k * (dir == 0 ? ci : co))) return pl;
  if (!fits_int((int64_t)t * n)) return pl;
  pl.status = DS2_OK;
  if (empty) return pl;   // wgrad of an empty batch: the outputs are overwritten with zeros
  pl.d = C1Dims{t, n, ci, co, k, s, p, to};
  const bool fast = fast_enabled();
  if (dir == 2) {
    pl.ws_bytes = wgrad_ws(ci, co, k, s, p, rows);
    if (fast && is_gemm(k, s, p)) {
      pl.path = DS2_C1_GEMM;
    } else if (fast && fast_wgrad(ci, co)) {
      pl.path = DS2_C1_WGRAD_H3;
      pl.nsplit = wgrad_split(ci, co, k, rows, &pl.kchunk);
      pl.gx = cdiv((int64_t)k * ci, CT), pl.gy = cdiv(co, CT), pl.gz = pl.nsplit;
      pl.amax_passes = amax_given ? 1 : 2;
    } else {
      pl.path = DS2_C1_GENERAL;
      pl.gx = cdiv((int64_t)ci * k, 64), pl.gy = cdiv(co, 64), pl.gz = 1;
    }
    return pl;
  }
  if (fast && is_gemm(k, s, p)) {
    pl.path = DS2_C1_GEMM;   // ds2_sgemm_ws takes any workspace, NULL included
    return pl;
  }
  if (fast && (dir == 0 ? fast_fwd(ci, co, k) : fast_dgrad(ci, co, k, s, p))) {
    if (dir == 1) pl.d = C1Dims{to, n, co, ci, k, 1, k - 1 - p, t};
    const C1Dims& d = pl.d;
    const int cip = pad32(d.ci);
    const int tm = d.t_in > d.t_out ? d.t_in : d.t_out;
    pl.path = d.ci % 4 == 0 && (x_addr & 15) == 0 ? DS2_C1_IGEMM_VEC : DS2_C1_IGEMM_SCALAR;
    pl.stages = d.k * (cip / CK);
    pl.gx = cdiv(d.co, CT), pl.gy = cdiv((int64_t)d.t_out * d.n, CT), pl.gz = 1;
    pl.ws_bytes = al256((size_t)d.co * d.k * cip * 4) + al256((size_t)tm * d.n * 4) +
                  al256((size_t)d.co * 4);
    pl.amax_passes = amax_given && dir == 0 ? 1 : 2;
    return pl;
  }
  pl.path = DS2_C1_GENERAL;
  pl.gx = cdiv(dir == 0 ? co : ci, 64), pl.gy = cdiv((dir == 0 ? rows : (int64_t)t * n), 64), pl.gz = 1;
  return pl;
}

template <int MODE>
ds2_status_t launch_general(const float* a, const float* b, const float* bias, float* c,
                            const C1Plan& pl, int64_t M, int64_t NN, int64_t K, hipStream_t st,
                            const char* where) {
  const dim3 grid(pl.gx, pl.gy);   // cdiv(NN, 64), cdiv(M, 64)
  hipLaunchKernelGGL((c1_general_kernel<MODE>), grid, dim3(256), 0, st, a, b, bias, c, pl.d, M, NN, K);
  return launch_status(where);
}

// forward, or dgrad as the forward of dy on the flipped weights (flip != 0: pl.d describes
// that convolution).  The workspace holds pl.ws_bytes (checked by the caller).
ds2_status_t run_igemm(const float* x, const float* w, const float* bias, float* y,
                       const C1Plan& pl, int flip, const unsigned* x_rmax_in, void* ws,
                       hipStream_t st, const char* where) {
  const C1Dims& d = pl.d;
  const int cip = pad32(d.ci);
  const int tm = d.t_in > d.t_out ? d.t_in : d.t_out;
  const size_t b_w = al256((size_t)d.co * d.k * cip * 4), b_r = al256((size_t)tm * d.n * 4);
  char* base = static_cast<char*>(ws);
  float* wr = reinterpret_cast<float*>(base);
  const unsigned* x_rmax = x_rmax_in != nullptr ? x_rmax_in : reinterpret_cast<unsigned*>(base + b_w);
  unsigned* w_rmax = reinterpret_cast<unsigned*>(base + b_w + b_r);
  const int64_t wtot = (int64_t)d.co * d.k * cip;
  // w is [Cout][Cin][k] of the real convolution: for flip its rows are d.ci, columns d.co
  hipLaunchKernelGGL(c1_relayout_w_kernel, dim3(ew_grid(wtot)), dim3(256), 0, st, w,
                     flip ? d.ci : d.co, flip ? d.co : d.ci, d.k, cip, flip, wr);
  hipLaunchKernelGGL(c1_rowmax_kernel, dim3(cdiv(d.co, 4)), dim3(256), 0, st, wr, d.co, d.k * cip,
                     w_rmax);
  const int xr = d.t_in * d.n;
  if (x_rmax_in == nullptr)   // else: the producer of x left its row maxima
    hipLaunchKernelGGL(c1_rowmax_kernel, dim3(cdiv(xr, 4)), dim3(256), 0, st, x, xr, d.ci,
                       reinterpret_cast<unsigned*>(base + b_w));
  const dim3 grid(pl.gx, pl.gy);
  if (pl.path == DS2_C1_IGEMM_VEC)
    hipLaunchKernelGGL((c1_igemm_kernel<true>), grid, dim3(256), 0, st, x, wr, bias, y, x_rmax,
                       w_rmax, d, cip);
  else
    hipLaunchKernelGGL((c1_igemm_kernel<false>), grid, dim3(256), 0, st, x, wr, bias, y, x_rmax,
                       w_rmax, d, cip);
  return launch_status(where);
}

// ---------------------------------------------------------------------------
// pointwise
__global__ __launch_bounds__(256) void glu_fwd_kernel(const float* __restrict__ x, int64_t rows,
                                                      int c, float* __restrict__ y) {
  const int64_t total = rows * c;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / c;
    const int j = (int)(i - r * c);
    const float* xr = x + r * 2 * c;
    y[i] = xr[j] * sigmoidf_(xr[c + j]);
  }
}

__global__ __launch_bounds__(256) void glu_bwd_kernel(const float* __restrict__ dy,
                                                      const float* __restrict__ x, int64_t rows,
                                                      int c, float* __restrict__ dx) {
  const int64_t total = rows * c;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / c;
    const int j = (int)(i - r * c);
    const float* xr = x + r * 2 * c;
    const float a = xr[j], sg = sigmoidf_(xr[c + j]), g = dy[i];
    dx[r * 2 * c + j] = g * sg;
    dx[r * 2 * c + c + j] = g * a * sg * (1.f - sg);
  }
}

__global__ __launch_bounds__(256) void bn_relu_kernel(const float* __restrict__ x, int64_t rows,
                                                      int c, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta,
                                                      float* __restrict__ y) {
  const int64_t total = rows * c;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % c);
    // the expression of bn.hip's apply kernels, then the ReLU
    const float v = gamma[j] * ((x[i] - mean[j]) * invstd[j]) + beta[j];
    y[i] = v > 0.f ? v : 0.f;
  }
}

// float4 form (c % 4 == 0, 16-B aligned operands)
__global__ __launch_bounds__(256) void bn_relu4_kernel(const float4* __restrict__ x, int64_t rows,
                                                       int c4, const float4* __restrict__ mean,
                                                       const float4* __restrict__ invstd,
                                                       const float4* __restrict__ gamma,
                                                       const float4* __restrict__ beta,
                                                       float4* __restrict__ y) {
  const int64_t total = rows * c4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % c4);
    const float4 v = x[i], m = mean[j], s = invstd[j], g = gamma[j], b = beta[j];
    float4 o;
    o.x = fmaxf(g.x * ((v.x - m.x) * s.x) + b.x, 0.f);
    o.y = fmaxf(g.y * ((v.y - m.y) * s.y) + b.y, 0.f);
    o.z = fmaxf(g.z * ((v.z - m.z) * s.z) + b.z, 0.f);
    o.w = fmaxf(g.w * ((v.w - m.w) * s.w) + b.w, 0.f);
    y[i] = o;
  }
}

// x [n][c][t] -> y [t][n][c]: 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void nct_to_tnc_kernel(const float* __restrict__ x, int n, int c,
                                                         int t, float* __restrict__ y) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cc = c0 + ty + 8 * i, tt = t0 + tx;
    if (cc < c && tt < t) tile[ty + 8 * i][tx] = x[((int64_t)b * c + cc) * t + tt];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int tt = t0 + ty + 8 * i, cc = c0 + tx;
    if (cc < c && tt < t) y[((int64_t)tt * n + b) * c + cc] = tile[tx][ty + 8 * i];
  }
}

// dz = dy where the ReLU passed (y > 0), else 0
__global__ __launch_bounds__(256) void relu_mask_kernel(const float* __restrict__ dy,
                                                        const float* __restrict__ y, int64_t total,
                                                        float* __restrict__ dz) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    dz[i] = y[i] > 0.f ? dy[i] : 0.f;
}

}  // namespace
}  // namespace ds2

using namespace ds2;

extern "C" {

size_t ds2_conv1d_workspace_size(int t, int n, int c_in, int c_out, int k, int s, int p) {
  if (!dims_ok(t, n, c_in, c_out, k, s, p)) return 0;
  if (t + 2 * p - k < 0 && t != 0 && n != 0) return 0;   // the entry points reject the shape
  const int to = out_len(t, k, s, p);
  size_t b = fwd_ws_fast(t, n, c_in, c_out, k, to);
  if (is_gemm(k, s, p) && fits_int((int64_t)t * n)) {
    const size_t gf = ds2_sgemm_workspace_size(t * n, c_out, c_in, 1);
    const size_t gd = ds2_sgemm_workspace_size(t * n, c_in, c_out, 1);
    if (gf > b) b = gf;
    if (gd > b) b = gd;
  }
  return b + 256;
}

ds2_status_t ds2_conv1d_fwd(const float* x, const float* w, const float* bias, float* y, int t,
                            int n, int c_in, int c_out, int k, int s, int p, void* ws,
                            size_t ws_bytes, ds2_stream_t stream) {
  return ds2_conv1d_fwd_amax(x, w, bias, y, t, n, c_in, c_out, k, s, p, nullptr, ws, ws_bytes,
                             stream);
}

ds2_status_t ds2_conv1d_fwd_amax(const float* x, const float* w, const float* bias, float* y,
                                 int t, int n, int c_in, int c_out, int k, int s, int p,
                                 const unsigned* x_row_amax, void* ws, size_t ws_bytes,
                                 ds2_stream_t stream) {
  const C1Plan pl = c1_plan(0, t, n, c_in, c_out, k, s, p, reinterpret_cast<uintptr_t>(x),
                            x_row_amax != nullptr);
  if (pl.status != DS2_OK || pl.path == DS2_C1_NONE) return pl.status;
  if (x == nullptr || w == nullptr || y == nullptr) return DS2_INVALID_VALUE;
  if (pl.ws_bytes != 0 && (ws == nullptr || ws_bytes < pl.ws_bytes)) return DS2_WORKSPACE_TOO_SMALL;
  const int64_t M = (int64_t)pl.d.t_out * n;
  hipStream_t st = as_stream(stream);
  switch (pl.path) {
    case DS2_C1_GEMM:
      return ds2_sgemm_ws(0, 1, (int)M, c_out, c_in, 1.f, x, c_in, 0, w, c_in, 0, 0.f, y, c_out, 0, 1,
                          bias, ws, ws_bytes, stream);
    case DS2_C1_IGEMM_VEC:
    case DS2_C1_IGEMM_SCALAR:
      return run_igemm(x, w, bias, y, pl, 0, x_row_amax, ws, st, "ds2_conv1d_fwd");
    default:
      return launch_general<0>(x, w, bias, y, pl, M, c_out, (int64_t)k * c_in, st, "ds2_conv1d_fwd");
  }
}

ds2_status_t ds2_conv1d_dgrad(const float* dy, const float* w, float* dx, int t, int n, int c_in,
                              int c_out, int k, int s, int p, void* ws, size_t ws_bytes,
                              ds2_stream_t stream) {
  const C1Plan pl = c1_plan(1, t, n, c_in, c_out, k, s, p, reinterpret_cast<uintptr_t>(dy), false);
  if (pl.status != DS2_OK || pl.path == DS2_C1_NONE) return pl.status;
  if (dy == nullptr || w == nullptr || dx == nullptr) return DS2_INVALID_VALUE;
  if (pl.ws_bytes != 0 && (ws == nullptr || ws_bytes < pl.ws_bytes)) return DS2_WORKSPACE_TOO_SMALL;
  const int64_t M = (int64_t)t * n;
  hipStream_t st = as_stream(stream);
  switch (pl.path) {
    case DS2_C1_GEMM:
      return ds2_sgemm_ws(0, 0, (int)M, c_in, c_out, 1.f, dy, c_out, 0, w, c_in, 0, 0.f, dx, c_in, 0,
                          1, nullptr, ws, ws_bytes, stream);
    case DS2_C1_IGEMM_VEC:
    case DS2_C1_IGEMM_SCALAR:
      return run_igemm(dy, w, nullptr, dx, pl, 1, nullptr, ws, st, "ds2_conv1d_dgrad");
    default:
      return launch_general<1>(dy, w, nullptr, dx, pl, M, c_in, (int64_t)k * c_out, st,
                               "ds2_conv1d_dgrad");
  }
}

size_t ds2_conv1d_wgrad_workspace_size(int t, int n, int c_in, int c_out, int k, int s, int p) {
  if (!dims_ok(t, n, c_in, c_out, k, s, p)) return 0;
  if (t + 2 * p - k < 0 && t != 0 && n != 0) return 0;   // the entry point rejects the shape
  const int to = out_len(t, k, s, p);
  const int64_t rows = (int64_t)to * n;
  if (!fits_int(rows)) return 0;
  return wgrad_ws(c_in, c_out, k, s, p, rows);
}

ds2_status_t ds2_conv1d_wgrad(const float* dy, const float* x, float* dw, float* dbias, int t, int n,
                              int c_in, int c_out, int k, int s, int p, void* ws, size_t ws_bytes,
                              ds2_stream_t stream) {
  return ds2_conv1d_wgrad_amax(dy, x, dw, dbias, t, n, c_in, c_out, k, s, p, nullptr, ws, ws_bytes,
                               stream);
}

ds2_status_t ds2_conv1d_wgrad_amax(const float* dy, const float* x, float* dw, float* dbias, int t,
                                   int n, int c_in, int c_out, int k, int s, int p,
                                   const unsigned* x_col_amax, void* ws, size_t ws_bytes,
                                   ds2_stream_t stream) {
  const C1Plan pl = c1_plan(2, t, n, c_in, c_out, k, s, p, 0, x_col_amax != nullptr);
  if (pl.status != DS2_OK) return pl.status;
  hipStream_t st = as_stream(stream);
  if (pl.path == DS2_C1_NONE) {   // an empty batch: the outputs are overwritten with the empty sum
    if ((dw != nullptr && hipMemsetAsync(dw, 0, (size_t)c_out * c_in * k * 4, st) != hipSuccess) ||
        (dbias != nullptr && hipMemsetAsync(dbias, 0, (size_t)c_out * 4, st) != hipSuccess))
      return launch_status("ds2_conv1d_wgrad");
    return DS2_OK;
  }
  if (dy == nullptr || x == nullptr || dw == nullptr) return DS2_INVALID_VALUE;
  if (ws == nullptr || ws_bytes < pl.ws_bytes) return DS2_WORKSPACE_TOO_SMALL;
  const C1Dims& d = pl.d;
  const int64_t rows = (int64_t)d.t_out * n;
  const size_t head = al256(wgrad_ws_head(c_in, c_out, k, s, p, rows));
  char* base = static_cast<char*>(ws);
  if (dbias != nullptr) {
    const ds2_status_t e = ds2_colsum(dy, (int)rows, c_out, c_out, dbias, 0, base, head, stream);
    if (e != DS2_OK) return e;
  }
  switch (pl.path) {
    case DS2_C1_GEMM:
      return ds2_sgemm_ws(1, 0, c_out, c_in, (int)rows, 1.f, dy, c_out, 0, x, c_in, 0, 0.f, dw, c_in,
                          0, 1, nullptr, base, head, stream);
    case DS2_C1_WGRAD_H3: {
      unsigned* x_cmax = reinterpret_cast<unsigned*>(base + head);
      unsigned* dy_cmax = reinterpret_cast<unsigned*>(base + head + al256((size_t)c_in * 4));
      float* part = reinterpret_cast<float*>(base + head + al256((size_t)c_in * 4) +
                                             al256((size_t)c_out * 4));
      if (hipMemsetAsync(x_cmax, 0, al256((size_t)c_in * 4) + al256((size_t)c_out * 4), st) != hipSuccess)
        return launch_status("ds2_conv1d_wgrad");
      if (x_col_amax == nullptr)   // else: the producer of x left its column maxima
        hipLaunchKernelGGL(c1_colmax_kernel, dim3(cdiv((int64_t)t * n, 128)), dim3(256), 0, st, x,
                           t * n, c_in, x_cmax);
      hipLaunchKernelGGL(c1_colmax_kernel, dim3(cdiv(rows, 128)), dim3(256), 0, st, dy, (int)rows,
                         c_out, dy_cmax);
      hipLaunchKernelGGL(c1_wgrad_kernel, dim3(pl.gx, pl.gy, pl.gz), dim3(256), 0, st, dy, x, part,
                         dy_cmax, x_col_amax != nullptr ? x_col_amax : x_cmax, d, pl.kchunk);
      const int64_t tot = (int64_t)c_out * c_in * k;
      hipLaunchKernelGGL(c1_wgrad_reduce_kernel, dim3(ew_grid(tot)), dim3(256), 0, st, part,
                         pl.nsplit, c_out, c_in, k, dw);
      return launch_status("ds2_conv1d_wgrad");
    }
    default:
      return launch_general<2>(dy, x, nullptr, dw, pl, c_out, (int64_t)c_in * k, rows, st,
                               "ds2_conv1d_wgrad");
  }
}

ds2_status_t ds2_test_conv1d_plan(int dir, int t, int n, int c_in, int c_out, int k, int s, int p,
                                  unsigned long long x_addr, int* out) {
  if (dir < 0 || dir > 6 || (dir & 3) == 3 || out == nullptr) return DS2_INVALID_VALUE;
  const C1Plan pl = c1_plan(dir & 3, t, n, c_in, c_out, k, s, p, (uintptr_t)x_addr, (dir & 4) != 0);
  if (pl.status != DS2_OK) return pl.status;
  const int vals[10] = {pl.path, pl.stages, (int)pl.gx, (int)pl.gy, (int)pl.gz, pl.nsplit, pl.kchunk,
                        static_cast<int>(pl.ws_bytes & 0xffffffffu),
                        static_cast<int>((uint64_t)pl.ws_bytes >> 32), pl.amax_passes};
  for (int i = 0; i < 10; ++i) out[i] = vals[i];
  return DS2_OK;
}

ds2_status_t ds2_nct_to_tnc(const float* x, int n, int c, int t, float* y, ds2_stream_t stream) {
  if (n < 0 || c < 0 || t < 0 || n > 65535) return DS2_INVALID_VALUE;
  if (n == 0 || c == 0 || t == 0) return DS2_OK;
  hipLaunchKernelGGL(nct_to_tnc_kernel, dim3(cdiv(t, 32), cdiv(c, 32), n), dim3(256), 0,
                     as_stream(stream), x, n, c, t, y);
  return launch_status("ds2_nct_to_tnc");
}

ds2_status_t ds2_glu_fwd(const float* x, int rows, int c, float* y, ds2_stream_t stream) {
  if (rows < 0 || c < 0) return DS2_INVALID_VALUE;
  const int64_t total = (int64_t)rows * c;
  if (total == 0) return DS2_OK;
  hipLaunchKernelGGL(glu_fwd_kernel, dim3(ew_grid(total)), dim3(256), 0, as_stream(stream), x,
                     (int64_t)rows, c, y);
  return launch_status("ds2_glu_fwd");
}

ds2_status_t ds2_glu_bwd(const float* dy, const float* x, int rows, int c, float* dx,
                         ds2_stream_t stream) {
  if (rows < 0 || c < 0) return DS2_INVALID_VALUE;
  const int64_t total = (int64_t)rows * c;
  if (total == 0) return DS2_OK;
  hipLaunchKernelGGL(glu_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, as_stream(stream), dy, x,
                     (int64_t)rows, c, dx);
  return launch_status("ds2_glu_bwd");
}

ds2_status_t ds2_bn_relu_apply(const float* x, int rows, int c, const float* mean,
                               const float* invstd, const float* gamma, const float* beta, float* y,
                               ds2_stream_t stream) {
  if (rows < 0 || c < 0) return DS2_INVALID_VALUE;
  const int64_t total = (int64_t)rows * c;
  if (total == 0) return DS2_OK;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) |
                         reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(invstd) |
                         reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta);
  if (c % 4 == 0 && (bits & 15) == 0)
    hipLaunchKernelGGL(bn_relu4_kernel, dim3(ew_grid(total / 4)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4*>(x), (int64_t)rows, c / 4,
                       reinterpret_cast<const float4*>(mean), reinterpret_cast<const float4*>(invstd),
                       reinterpret_cast<const float4*>(gamma), reinterpret_cast<const float4*>(beta),
                       reinterpret_cast<float4*>(y));
  else
    hipLaunchKernelGGL(bn_relu_kernel, dim3(ew_grid(total)), dim3(256), 0, as_stream(stream), x,
                       (int64_t)rows, c, mean, invstd, gamma, beta, y);
  return launch_status("ds2_bn_relu_apply");
}

ds2_status_t ds2_bn_relu_apply_amax(const float* x, int rows, int c, const float* mean,
                                    const float* invstd, const float* gamma, const float* beta,
                                    float* y, unsigned* row_amax, unsigned* col_amax,
                                    ds2_stream_t stream) {
  if (rows < 0 || c < 0) return DS2_INVALID_VALUE;
  if (row_amax == nullptr || col_amax == nullptr) return DS2_INVALID_VALUE;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) |
                         reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(invstd) |
                         reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta);
  if (c % 4 != 0 || c > 2048 || (bits & 15) != 0) return DS2_UNSUPPORTED_SHAPE;
  if (rows == 0 || c == 0) return DS2_OK;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(col_amax, 0, (size_t)c * 4, st) != hipSuccess)
    return launch_status("ds2_bn_relu_apply_amax");
  launch_rows_amax<true, true>(x, rows, c, c, mean, invstd, gamma, beta, y, row_amax, col_amax, st);
  return launch_status("ds2_bn_relu_apply_amax");
}

size_t ds2_bn_relu_bwd_workspace_size(int rows, int c) {
  if (rows < 0 || c < 0) return 0;
  return al256((size_t)rows * c * 4) + ds2_bn_workspace_size(rows, c, 1) + 256;
}

ds2_status_t ds2_bn_relu_bwd(const float* dy, const float* y, const float* x, int rows, int c,
                             const float* mean, const float* invstd, const float* gamma,
                             const float* beta, float* dx, float* dgamma, float* dbeta, void* ws,
                             size_t ws_bytes, ds2_stream_t stream) {
  if (rows < 0 || c < 0) return DS2_INVALID_VALUE;
  const int64_t total = (int64_t)rows * c;
  if (total == 0) return DS2_OK;
  if (ws == nullptr || ws_bytes < ds2_bn_relu_bwd_workspace_size(rows, c))
    return DS2_WORKSPACE_TOO_SMALL;
  float* dz = static_cast<float*>(ws);
  const size_t off = al256((size_t)total * 4);
  hipLaunchKernelGGL(relu_mask_kernel, dim3(ew_grid(total)), dim3(256), 0, as_stream(stream), dy, y,
                     total, dz);
  const ds2_status_t e = launch_status("ds2_bn_relu_bwd");
  if (e != DS2_OK) return e;
  return ds2_bn_backward(dz, 0, x, rows, c, 1, 1, mean, invstd, gamma, beta, 0, nullptr, 0.f, 0.f,
                         /*eps: not known here, the stored invstd at every count*/ 0.f, dx, dgamma,
                         dbeta, nullptr, static_cast<char*>(ws) + off, ws_bytes - off, stream);
}

}  // extern "C"
