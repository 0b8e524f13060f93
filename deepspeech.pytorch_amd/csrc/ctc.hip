// CTC loss (warp-ctc semantics) and greedy CTC decoding.
//
// CTC: one workgroup per utterance.  log-softmax rows are materialised once in
// the workspace; alpha is scanned forward (one LDS row per step, stored to the
// workspace), beta is scanned backward keeping only the current LDS row, and the
// gradient row for frame t is produced right after beta_t is known:
//   grad[t][c] = softmax[t][c] - sum_{s: l'_s = c} exp(alpha_t(s) + beta_t(s) + nll - lp[t][c])
// which is d(-log p)/d(acts) through the internal softmax (ref: warpctc_pytorch,
// called at train.py:600-602; torch's ctc_loss backward formula is identical).
// Per-class sums walk a per-utterance class->state list in LDS, so results are
// deterministic (no float atomics).
//
// Forced alignment (ds2_ctc_align): the max-plus form of the alpha scan with one back-pointer
// byte per (t, s) and a back-trace staged through LDS; see ctc_align_kernel.
//
// Greedy: one wave per utterance; argmax (first maximum) per frame, then a
// ballot/mbcnt compaction of the frames that survive blank/repeat removal
// (ref decoder.py:165-197).
#include <type_traits>
#include "common.h"
#include "../../include/ds2hip_test.h"

namespace ds2 {

constexpr int kScanThreads = 512;
constexpr int kMaxLabel = 1024;
constexpr int kCtcMaxS = 2 * kMaxLabel + 1;

__device__ __forceinline__ int label_at(const int* lab, int s, int blank) {
  return (s & 1) ? lab[s >> 1] : blank;
}

struct CtcWs {
  float* lp;         // [n][t_max][c]       log-softmax
  float* alpha;      // [n][t_max][s_max]
  float* beta;       // [n][t_max][s_max]
  double* nll;       // [n]
  double* shift;     // [2][n][t_max]       the row maxima subtracted by the alpha / beta scans
  int* offs;         // [n]                 label offsets
  int* cls_start;    // [n][65]             per-class start into cls_pos
  int* cls_pos;      // [n][max_label_len]  label positions grouped by class
};

// 1) log-softmax of every (t, n) row, one wave per row (C <= 64).  kFromMax (the alignment;
//    the loss keeps v - lse bit for bit): (v - m) - log1p(sum over the classes but the first
//    maximum), which has no cancellation at |m|: v - lse rounds lse to an ulp of |m| (1e-6 at
//    12), an absolute error per frame that a peaked row's log-probability (-1e-4) and a score
//    summed over hundreds of such frames cannot absorb.
template <bool kFromMax>
__global__ void ctc_logsoftmax_kernel(const float* __restrict__ acts, int t_max, int n, int c,
                                      float* __restrict__ lp) {
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;   // row = t*n + b
  const int lane = threadIdx.x & 63;
  if (row >= t_max * n) return;
  const int t = row / n;
  const int b = row - t * n;
  const float v = lane < c ? acts[(int64_t)row * c + lane] : -INFINITY;
  const float m = wave_max(v);
  if constexpr (kFromMax) {
    const int first = __ffsll(static_cast<long long>(__ballot(v == m))) - 1;
    const float e = (lane < c && lane != first) ? expf(v - m) : 0.f;
    const float l1p = log1pf(wave_sum(e));
    if (lane < c) lp[((int64_t)b * t_max + t) * c + lane] = (v - m) - l1p;
  } else {
    const float e = lane < c ? expf(v - m) : 0.f;
    const float lse = m + logf(wave_sum(e));
    if (lane < c) lp[((int64_t)b * t_max + t) * c + lane] = v - lse;
  }
}

// 2) per utterance: label offset and the class -> label-position lists
__global__ __launch_bounds__(64) void ctc_prep_kernel(
    const int* __restrict__ labels, const int* __restrict__ label_lens, int n, int c, int max_l,
    int* __restrict__ offs, int* __restrict__ cls_start, int* __restrict__ cls_pos) {
  // one wave per utterance; lane k owns class k (c <= 64)
  __shared__ int lab_s[kMaxLabel];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  int part = 0;
  for (int i = lane; i < b; i += 64) part += label_lens[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  const int off = part;
  const int L = min(label_lens[b], kMaxLabel);   // host: label lengths <= max_l <= kMaxLabel
  for (int i = lane; i < L; i += 64) lab_s[i] = labels[off + i];
  __syncthreads();
  int cnt = 0;
  for (int i = 0; i < L; ++i) cnt += lab_s[i] == lane;
  int incl = cnt;                           // inclusive scan over the classes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  const int start = incl - cnt;             // labels of a smaller class
  if (lane == 0) offs[b] = off;
  int* cs = cls_start + b * 65;
  if (lane <= c) cs[lane] = start;
  if (lane == 0 && c == 64) cs[64] = L;
  int* cp = cls_pos + (int64_t)b * max_l;
  int w = start;
  for (int i = 0; i < L; ++i)
    if (lab_s[i] == lane) cp[w++] = i;
}

// 3) alpha (blockIdx.y == 0) and beta (blockIdx.y == 1) scans run concurrently,
//    one workgroup each per utterance; one LDS row per time step.  The utterance's
//    log-softmax rows are staged into LDS kScanChunk frames at a time, so the per-step
//    loop issues no global loads: a load there made the waitcnt pass wait for the
//    previous steps' alpha/beta row stores every step (1.1-1.3 us per step).  A thread
//    owns the states s = tid + kScanThreads * k; their labels and skip-transition flags
//    are computed once.  Every kScanRescale-th row is stored minus the previous row's maximum
//    (the per-wave maxima meet in LDS behind the step's barrier, so no extra barrier), and the
//    subtracted amounts are summed in fp64 per frame (`shift`).  The stored
//    values stay O(1-10) instead of growing to ~|log p| (~1e3 at T' = 501), whose fp32 ulp
//    (~1e-4) was a uniform relative error of every gradient term exp(alpha + beta + nll - lp).
constexpr int kScanPer = (kCtcMaxS + kScanThreads - 1) / kScanThreads;

// rows between rescalings: the row maximum falls by ~|log p| / T' per step (~3 for random
// logits), so the stored values stay within ~30 of zero; rescaling every step cost 0.2-0.35 us
// of each step's critical path (the reduction sits between the row and the barrier)
constexpr int kScanRescale = 8;

// wave maximum in VALU only (the DPP sequence of wave_min_dpp below): the scan's per-step row
// maximum; a shuffle chain (six ds_bpermute round trips) cost ~0.35 us per step there
template <int CTRL, int RMASK>
__device__ __forceinline__ float dpp_max_step(float x) {
  const int y = __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x),
                                            CTRL, RMASK, 0xf, false);
  return fmaxf(x, __builtin_bit_cast(float, y));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = dpp_max_step<0xB1, 0xf>(v);    // quad_perm [1, 0, 3, 2]
  v = dpp_max_step<0x4E, 0xf>(v);    // quad_perm [2, 3, 0, 1]
  v = dpp_max_step<0x141, 0xf>(v);   // row_half_mirror
  v = dpp_max_step<0x140, 0xf>(v);   // row_mirror
  v = dpp_max_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1, 3
  v = dpp_max_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
constexpr int kScanChunk = 256;        // frames of log probs per LDS stage (C <= 64)

__global__ __launch_bounds__(kScanThreads) void ctc_scan_kernel(
    const float* __restrict__ lp_all, int t_max, int c, const int* __restrict__ labels,
    const int* __restrict__ label_lens, const int* __restrict__ act_lens,
    const int* __restrict__ offs, int blank, int s_max, float* __restrict__ alpha_all,
    float* __restrict__ beta_all, double* __restrict__ shift_all, double* __restrict__ nll_out) {
  __shared__ float rows[2][kCtcMaxS];
  __shared__ float wmax[2][kScanThreads / 64];
  __shared__ int lab_s[kMaxLabel];
  __shared__ float lpc[kScanChunk * 64];
  const int b = blockIdx.x;
  const bool is_beta = blockIdx.y == 1;
  const int tid = threadIdx.x;
  const int L = label_lens[b];
  int T = act_lens[b];
  T = T > t_max ? t_max : (T < 0 ? 0 : T);
  const int S = 2 * L + 1;
  for (int i = tid; i < L; i += blockDim.x) lab_s[i] = labels[offs[b] + i];
  __syncthreads();
  const float* lp = lp_all + (int64_t)b * t_max * c;
  float* out = (is_beta ? beta_all : alpha_all) + (int64_t)b * t_max * s_max;
  double* shift = shift_all + ((int64_t)blockIdx.y * gridDim.x + b) * t_max;
  int ls[kScanPer];
  bool skip[kScanPer];
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int st = tid + kScanThreads * k;
    ls[k] = st < S ? label_at(lab_s, st, blank) : blank;
    const int o = is_beta ? st + 2 : st - 2;
    skip[k] = st < S && o >= 0 && o < S && ls[k] != blank && ls[k] != label_at(lab_s, o, blank);
  }
  int cur = 0;
  int f0 = 0, f1 = 0;                  // frames [f0, f1) staged in lpc
  double off = 0.0;                    // the row maxima subtracted so far (true = stored + off)
  for (int step = 0; step < T; ++step) {
    const int t = is_beta ? T - 1 - step : step;
    if (t < f0 || t >= f1) {           // uniform: stage the next chunk of frames
      f0 = is_beta ? max(0, t + 1 - kScanChunk) : t;
      f1 = is_beta ? t + 1 : min(T, t + kScanChunk);
      const int cnt = (f1 - f0) * c;
      for (int i = tid; i < cnt; i += kScanThreads) lpc[i] = lp[(int64_t)f0 * c + i];
      __syncthreads();
    }
    const float* lpt = lpc + (t - f0) * c;
    const float* prv = rows[cur ^ 1];
    float msub = 0.f;                  // the previous row's maximum, subtracted from this row
    if (step > 0 && (step & (kScanRescale - 1)) == 0) {
      float m = wmax[cur ^ 1][0];
#pragma unroll
      for (int w = 1; w < kScanThreads / 64; ++w) m = fmaxf(m, wmax[cur ^ 1][w]);
      msub = m == -INFINITY ? 0.f : m;
      off += msub;
    }
    float lm = -INFINITY;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      const int st = tid + kScanThreads * k;
      if (st >= S) break;
      float v;
      if (step == 0) {
        v = (is_beta ? st >= S - 2 : st <= 1) ? lpt[ls[k]] : -INFINITY;
      } else {
        const int d = is_beta ? 1 : -1;
        v = prv[st];
        if (st + d >= 0 && st + d < S) v = log_add_fast(v, prv[st + d]);
        if (skip[k]) v = log_add_fast(v, prv[st + 2 * d]);
        v = (v == -INFINITY) ? -INFINITY : v + (lpt[ls[k]] - msub);
      }
      lm = fmaxf(lm, v);
      rows[cur][st] = v;
      out[(int64_t)t * s_max + st] = v;
    }
    if ((step & (kScanRescale - 1)) == kScanRescale - 1) {   // uniform
      lm = wave_max_dpp(lm);
      if ((tid & 63) == 0) wmax[cur][tid >> 6] = lm;
    }
    if (tid == 0) shift[t] = off;
    __syncthreads();
    cur ^= 1;
  }
  if (!is_beta && tid == 0) {
    double ll;
    if (T == 0) {
      ll = (L == 0) ? 0.0 : -INFINITY;
    } else {
      const float* last = rows[cur ^ 1];
      float v = last[S - 1];
      if (S >= 2) v = log_add(v, last[S - 2]);
      ll = v == -INFINITY ? -INFINITY : (double)v + off;
    }
    nll_out[b] = -ll;
  }
}

// 4) gradient rows, one wave per (t, n):
//    grad[t][n][k] = exp(lp_k) - sum_{s: l'_s = k} exp(alpha_t(s) + beta_t(s) + nll - lp_k)
//    blank states summed by the whole wave, label classes by lane k over its list.
__global__ void ctc_grad_kernel(int t_max, int n, int c, int blank, int zero_infinity,
                                const int* __restrict__ act_lens, const int* __restrict__ label_lens,
                                const float* __restrict__ lp_all, const float* __restrict__ alpha_all,
                                const float* __restrict__ beta_all, const double* __restrict__ shift_all,
                                const double* __restrict__ nll_all,
                                const int* __restrict__ cls_start, const int* __restrict__ cls_pos,
                                int s_max, int max_l, float* __restrict__ costs,
                                float* __restrict__ grads) {
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;   // row = t*n + b
  const int lane = threadIdx.x & 63;
  if (row >= t_max * n) return;
  const int t = row / n;
  const int b = row - t * n;
  int T = act_lens[b];
  T = T > t_max ? t_max : (T < 0 ? 0 : T);
  const double nll_d = nll_all[b];
  const bool feasible = (nll_d != INFINITY) && (nll_d == nll_d);
  if (t == 0 && lane == 0 && costs != nullptr)
    costs[b] = feasible ? (float)nll_d : (zero_infinity ? 0.f : INFINITY);
  if (grads == nullptr) return;
  float* g = grads + (int64_t)row * c;
  if (t >= T || !feasible) {
    if (lane < c) g[lane] = 0.f;
    return;
  }
  const int L = label_lens[b];
  const int S = 2 * L + 1;
  const float* lpt = lp_all + ((int64_t)b * t_max + t) * c;
  const float* al = alpha_all + ((int64_t)b * t_max + t) * s_max;
  const float* be = beta_all + ((int64_t)b * t_max + t) * s_max;
  // alpha_t + beta_t + nll = stored alpha + stored beta + (both row shifts + nll): the large
  // parts cancel in fp64, so the exponent's fp32 error is that of O(1) values
  const float nll = (float)(shift_all[(int64_t)b * t_max + t] +
                            shift_all[((int64_t)n + b) * t_max + t] + nll_d);
  const float lpb = lpt[blank];
  float accb = 0.f;
  for (int s = 2 * lane; s < S; s += 128) {
    const float ab = al[s] + be[s];
    if (ab != -INFINITY) accb += expf(ab + nll - lpb);
  }
  accb = wave_sum(accb);
  if (lane < c) {
    const float lpk = lpt[lane];
    float acc;
    if (lane == blank) {
      acc = accb;
    } else {
      acc = 0.f;
      const int* cs = cls_start + b * 65;
      const int* cp = cls_pos + (int64_t)b * max_l;
      for (int i = cs[lane]; i < cs[lane + 1]; ++i) {
        const int s = 2 * cp[i] + 1;
        const float ab = al[s] + be[s];
        if (ab != -INFINITY) acc += expf(ab + nll - lpk);
      }
    }
    g[lane] = expf(lpk) - acc;
  }
}

// ---------------------------------------------------------------------------
// CTC forced alignment (ds2_ctc_align): the max-plus form of the alpha scan above.  One
// workgroup per utterance, the same state ownership, log-probability staging and rescaling as
// ctc_scan_kernel (a uniform shift changes no argmax; the shifts are summed in fp64 for the
// score).  Per (t, s) one back-pointer byte (0 stay, 1 from s - 1, 2 from s - 2) goes to the
// workspace.  Tie rule: a predecessor replaces the best so far only if strictly greater, tried
// in the order stay, s - 1, s - 2; the final state is S - 1 unless v(S - 2) > v(S - 1).
// Back-trace: a path moves down by at most 2 states per frame, so the kAlignChunk frames
// that end in state s_hi only visit states [s_hi - 2 kAlignChunk, s_hi]: that window of their
// back-pointer rows is staged into LDS (in the log-probability stage's place) with every load
// in flight at once, one lane walks it (an LDS read per frame, no dependent global load), and
// all threads then write the chunk's states and the spans of the labels it shows.
constexpr int kAlignChunk = 128;                       // frames of back-pointers per LDS stage
constexpr int kAlignWinDw = kAlignChunk / 2 + 2;       // dwords of a staged row: 2 K + 1 states
                                                       // from a 4-byte aligned start
constexpr int kAlignPer = (kAlignChunk * kAlignWinDw + kScanThreads - 1) / kScanThreads;
static_assert((kAlignChunk * kAlignWinDw + kAlignChunk + 2) * 4 <= kScanChunk * 64 * 4,
              "the back-trace stage and its path slice take the log-probability stage's LDS");

__global__ __launch_bounds__(kScanThreads) void ctc_align_kernel(
    const float* __restrict__ lp_all, int t_max, int c, const int* __restrict__ labels,
    const int* __restrict__ label_lens, const int* __restrict__ act_lens,
    const int* __restrict__ offs, int blank, int max_l, int bp_stride,
    unsigned char* __restrict__ bp_all, int* __restrict__ states_all, int* __restrict__ spans_all,
    float* __restrict__ scores) {
  __shared__ float rows[2][kCtcMaxS];
  __shared__ float wmax[2][kScanThreads / 64];
  __shared__ int lab_s[kMaxLabel];
  __shared__ float lpc[kScanChunk * 64];
  __shared__ int s_cur, s_nxt;         // back-trace: the states at a chunk's last frame and after it
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int L = min(label_lens[b], max_l);   // host: label lengths <= max_l (rows hold 2 max_l + 1)
  int T = act_lens[b];
  T = T > t_max ? t_max : (T < 0 ? 0 : T);
  const int S = 2 * L + 1;
  const int off_l = offs[b];
  for (int i = tid; i < L; i += blockDim.x) lab_s[i] = labels[off_l + i];
  __syncthreads();
  const float* lp = lp_all + (int64_t)b * t_max * c;
  unsigned char* bp = bp_all + (int64_t)b * t_max * bp_stride;
  int* states = states_all + (int64_t)b * t_max;
  int* spans = spans_all + 2 * (int64_t)off_l;
  int ls[kScanPer];
  bool skip[kScanPer];
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int st = tid + kScanThreads * k;
    ls[k] = st < S ? label_at(lab_s, st, blank) : blank;
    skip[k] = st < S && st >= 2 && ls[k] != blank && ls[k] != label_at(lab_s, st - 2, blank);
  }
  int cur = 0;
  int f1 = 0;                          // frames [f0, f1) staged in lpc
  int f0 = 0;
  double off = 0.0;                    // the row maxima subtracted so far (true = stored + off)
  for (int t = 0; t < T; ++t) {
    if (t >= f1) {                     // uniform: stage the next chunk of frames
      f0 = t;
      f1 = min(T, t + kScanChunk);
      const int cnt = (f1 - f0) * c;
      for (int i = tid; i < cnt; i += kScanThreads) lpc[i] = lp[(int64_t)f0 * c + i];
      __syncthreads();
    }
    const float* lpt = lpc + (t - f0) * c;
    const float* prv = rows[cur ^ 1];
    float msub = 0.f;                  // the previous row's maximum, subtracted from this row
    if (t > 0 && (t & (kScanRescale - 1)) == 0) {
      float m = wmax[cur ^ 1][0];
#pragma unroll
      for (int w = 1; w < kScanThreads / 64; ++w) m = fmaxf(m, wmax[cur ^ 1][w]);
      msub = m == -INFINITY ? 0.f : m;
      off += msub;
    }
    float lm = -INFINITY;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      const int st = tid + kScanThreads * k;
      if (st >= S) break;
      float v;
      int d = 0;
      if (t == 0) {
        v = st <= 1 ? lpt[ls[k]] : -INFINITY;
      } else {
        v = prv[st];
        if (st >= 1) {
          const float u = prv[st - 1];
          if (u > v) { v = u; d = 1; }
        }
        if (skip[k]) {
          const float u = prv[st - 2];
          if (u > v) { v = u; d = 2; }
        }
        v = (v == -INFINITY) ? -INFINITY : v + (lpt[ls[k]] - msub);
      }
      lm = fmaxf(lm, v);
      rows[cur][st] = v;
      bp[(int64_t)t * bp_stride + st] = static_cast<unsigned char>(d);
    }
    if ((t & (kScanRescale - 1)) == kScanRescale - 1) {   // uniform
      lm = wave_max_dpp(lm);
      if ((tid & 63) == 0) wmax[cur][tid >> 6] = lm;
    }
    __syncthreads();
    cur ^= 1;
  }
  // the final state and the score; s_cur < 0: no alignment (or no frames)
  if (tid == 0) {
    int sf = -1;
    float sc = (T == 0 && L == 0) ? 0.f : -INFINITY;
    if (T > 0) {
      const float* last = rows[cur ^ 1];
      float v = last[S - 1];
      sf = S - 1;
      if (S >= 2 && last[S - 2] > v) { v = last[S - 2]; sf = S - 2; }
      if (v == -INFINITY) sf = -1;
      else sc = static_cast<float>((double)v + off);
    }
    scores[b] = sc;
    s_cur = sf;
    s_nxt = -1;
  }
  __syncthreads();                     // also: this workgroup's back-pointer stores are visible
  const bool feasible = s_cur >= 0;
  const int t_end = feasible ? T : 0;  // states [t_end, t_max) = -1
  for (int t = t_end + tid; t < t_max; t += kScanThreads) states[t] = -1;
  if (!feasible) {
    if (!(T == 0 && L == 0))
      for (int i = tid; i < 2 * L; i += kScanThreads) spans[i] = -1;
    return;
  }
  unsigned* win = reinterpret_cast<unsigned*>(lpc);
  const unsigned char* winb = reinterpret_cast<const unsigned char*>(lpc);
  int* path = reinterpret_cast<int*>(lpc) + kAlignChunk * kAlignWinDw;   // [nf + 2]
  const int sw = bp_stride >> 2;       // dwords of a back-pointer row
  for (int e1 = T; e1 > 0; e1 -= kAlignChunk) {
    const int e0 = max(0, e1 - kAlignChunk);
    const int nf = e1 - e0;
    const int s_hi = s_cur;
    const int w0 = max(0, s_hi - 2 * kAlignChunk) >> 2;
    // every load of the chunk issued before the first is stored: addresses are clamped into
    // the chunk's rows (a clamped dword is never walked), so no load sits behind a branch
    unsigned wr[kAlignPer];
#pragma unroll
    for (int q = 0; q < kAlignPer; ++q) {
      const int i = tid + kScanThreads * q;
      const int r = min(i / kAlignWinDw, nf - 1);
      const int j = i % kAlignWinDw;
      wr[q] = reinterpret_cast<const unsigned*>(bp + (int64_t)(e0 + r) * bp_stride)[
          min(w0 + j, sw - 1)];
    }
#pragma unroll
    for (int q = 0; q < kAlignPer; ++q) {
      const int i = tid + kScanThreads * q;
      if (i < nf * kAlignWinDw) win[i] = wr[q];
    }
    __syncthreads();
    if (tid == 0) {
      int s = s_hi;
      path[nf + 1] = s_nxt;
      for (int t = e1 - 1; t >= e0; --t) {
        path[t - e0 + 1] = s;
        const int d = winb[(t - e0) * (kAlignWinDw * 4) + (s - 4 * w0)];
        s = t > 0 ? s - min(d, s) : -1;
      }
      path[0] = s;                     // the state at frame e0 - 1 (-1 before the first frame)
      s_nxt = path[1];
      s_cur = s;
    }
    __syncthreads();
    for (int i = tid; i < nf; i += kScanThreads) {
      const int s = path[i + 1];
      states[e0 + i] = s;
      if (s & 1) {
        if (path[i] != s) spans[s - 1] = e0 + i;           // 2 * (s >> 1)
        if (path[i + 2] != s) spans[s] = e0 + i + 1;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
__global__ void greedy_kernel(const float* __restrict__ probs, int n, int t_max, int c,
                              int64_t stride_n, int64_t stride_t, const int* __restrict__ sizes,
                              int blank, int* __restrict__ out_ids, int* __restrict__ out_offsets,
                              int* __restrict__ out_counts, int* __restrict__ argmax_out) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= n) return;
  int size = sizes != nullptr ? sizes[wave] : t_max;
  if (size > t_max) size = t_max;
  if (size < 0) size = 0;
  const float* p = probs + (int64_t)wave * stride_n;
  int prev_last = -1;  // idx of frame (chunk_start - 1)
  int count = 0;
  for (int t0 = 0; t0 < t_max; t0 += 64) {
    const int t = t0 + lane;
    int idx = -1;
    if (t < t_max) {
      const float* row = p + (int64_t)t * stride_t;
      float best = row[0];
      idx = 0;
      for (int k = 1; k < c; ++k) {
        const float v = row[k];
        // torch.max semantics: first maximum; NaN counts as the maximum.
        if (best == best && (v > best || v != v)) {
          best = v;
          idx = k;
        }
      }
      if (argmax_out != nullptr) argmax_out[(int64_t)wave * t_max + t] = idx;
    }
    int prev = __shfl_up(idx, 1, 64);
    if (lane == 0) prev = prev_last;
    const bool emit = (t < size) && (idx != blank) && !(t > 0 && idx == prev);
    const unsigned long long mask = __ballot(emit);
    const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(mask >> 32),
                                               __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(mask), 0));
    if (emit) {
      out_ids[(int64_t)wave * t_max + count + rank] = idx;
      out_offsets[(int64_t)wave * t_max + count + rank] = t;
    }
    count += __popcll(mask);
    prev_last = __shfl(idx, 63, 64);
  }
  if (lane == 0) out_counts[wave] = count;
}


// ---------------------------------------------------------------------------
// CTC prefix beam search (BeamCTCDecoder, decoder.py:90-143, wrapping ctcdecode's
// ctc_beam_search_decoder; LM = true adds its KenLM Scorer, see BeamLm below).  One 64-lane
// workgroup per utterance; the beam (<= 128 prefixes) lives in LDS, the prefix
// trie (parent, char, timestep, best char log-prob) in the workspace.  Per frame:
// prune the vocabulary (cutoff_top_n / cutoff_prob), score every candidate
// (prefix x char: blank / repeat "stay" terms, extensions, extensions that land on a
// prefix already in the beam are merged into it), then keep the beam_width best by
// (score desc, last char asc, candidate index asc).  oracle/ctc_beam.py restates the
// same algorithm (parity with ctcdecode itself is unpinned: it is not available).
// Trie-node revival (path_trie.cpp get_path_trie / remove): a node pruned from the beam
// stays in the trie while a descendant is in the beam, and an extension onto it revives
// it.  Per node: cnt = (in the beam) + (children alive), km = the chars of its alive
// children, a child list (fc first child, ns next sibling); a pruned node whose cnt drops
// to 0 is dead and takes its bit out of its parent's km (and its count, recursively).
// km is loaded per frame, so the list walk runs only where a revival is attempted.
// two instantiations: beams <= 32 over vocabularies <= 64, and beams <= 128 (the
// reference's default beam_width is 100, decoder.py:89) over vocabularies <= 32 -- both
// keep every candidate (k = entry * C + char < 4096) in the wave's registers
constexpr int BEAM_SMALL = 32, BEAM_SMALL_C = 64;
constexpr int BEAM_LARGE = 128, BEAM_LARGE_C = 32;
// a third for beams of 33..128 over vocabularies of 33..64 (the reference's Cyrillic label
// set at its default beam): up to 8192 candidates, so the candidate index takes 13 bits of
// the key, a winner's pb / pnb are read back from its key and its entry's blank candidate
// instead of being stored per candidate, and more than 4096 candidates are selected per
// half (beam_select_half) and merged -- see DESIGN.md, "beams up to 128 over 33..64 labels"
constexpr int BEAM_WIDE = 128, BEAM_WIDE_C = 64;
constexpr int BEAM_WIDE_TCH = 64;   // its staging chunk
constexpr int BEAM_LDS_PER_CU = 160 * 1024;
// frames of probabilities staged in LDS at a time: a global load consumed inside the frame
// loop would make the waitcnt pass wait (vmcnt(0)) for the previous frame's trie stores
constexpr int BEAM_TCH = 128;

__device__ __forceinline__ float beam_lse(float a, float b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const float m = fmaxf(a, b);
  return logf(expf(a - m) + expf(b - m)) + m;
}

// lexicographic "better": higher score, then lower char, then lower candidate index
__device__ __forceinline__ bool beam_better(float s1, int key1, float s2, int key2) {
  return s1 > s2 || (s1 == s2 && key1 < key2);
}

// (score, key) packed so that beam_better is the unsigned 64-bit order: the score's bits made
// order-preserving in the high word (-0 read as +0, which beam_better calls equal), the key
// reversed in the low word; -inf and NaN (never selected) pack to 0, below every candidate
__device__ __forceinline__ unsigned long long beam_pack(float s, int key) {
  if (!(s > -INFINITY)) return 0ull;
  unsigned b = __float_as_uint(s + 0.0f);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (static_cast<unsigned long long>(b) << 32) | (0xFFFFFFFFu - static_cast<unsigned>(key));
}

// keep the best `beam` of the tot candidates whose packed keys are ukey[0, tot) (unique;
// 0 = no candidate): lane l holds keys l, l + 64, ... in NJ registers (NJ >= the filled slots;
// the rest hold 0).  A radix select finds the threshold: bit by bit from the top, the
// largest T with at least `beam` keys >= T -- each test is NJ v_cmp ballots and their popcounts,
// no cross-lane data movement -- stopping early once exactly `beam` keys are >= T.  The
// selected keys are compacted into sk[] (LDS) and each is ranked by counting the selected
// keys above it, so sel_k receives the winners' candidate indices in rank order (the order
// of beam_better: score, then char, then index).  Returns the number selected.
template <int NJ, unsigned KMASK = 4095u>
__device__ __forceinline__ int beam_select(const unsigned long long* ukey, int tot, int beam,
                                           int* sel_k, unsigned long long* sk, int lane,
                                           unsigned long long lb) {
  unsigned long long ru[NJ];
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    const int k = lane + 64 * jj;
    ru[jj] = k < tot ? ukey[k] : 0ull;
  }
  auto count_ge = [&](unsigned long long c) {
    int n = 0;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) n += __popcll(__ballot(ru[jj] >= c));
    return n;
  };
  // fast path: lb (a key such that at least `beam` keys are >= it; 0 = none) usually leaves
  // at most 64 keys; they are compacted one per lane and ranked against each other by
  // v_readlane, with no bit-by-bit descent
  if (lb != 0ull) {
    const int ns = count_ge(lb);
    if (ns >= beam && ns <= 64) {
      int base = 0;
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const bool sel = ru[jj] >= lb;
        const unsigned long long m = __ballot(sel);
        if (sel)
          sk[base + __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                              __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0))] = ru[jj];
        base += __popcll(m);
      }
      __builtin_amdgcn_wave_barrier();
      const unsigned long long kr = lane < ns ? sk[lane] : 0ull;
      const unsigned klo = static_cast<unsigned>(kr), khi = static_cast<unsigned>(kr >> 32);
      int rank = 0;
      for (int j = 0; j < ns; ++j) {
        const unsigned long long kj =
            (static_cast<unsigned long long>(__builtin_amdgcn_readlane(khi, j)) << 32) |
            static_cast<unsigned>(__builtin_amdgcn_readlane(klo, j));
        rank += kj > kr ? 1 : 0;
      }
      if (lane < ns && rank < beam)
        sel_k[rank] = static_cast<int>((0xFFFFFFFFu - klo) & KMASK);
      return beam;
    }
  }
  unsigned long long thr = 1ull;                  // every candidate, when at most `beam`
  if (count_ge(1ull) > beam) {
    unsigned long long t = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
      const unsigned long long c = t | (1ull << bit);
      const int n = count_ge(c);
      if (n >= beam) {
        t = c;
        if (n == beam) break;
      }
    }
    thr = t;
  }
  int nsel = 0;
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    const bool sel = ru[jj] >= thr;
    const unsigned long long m = __ballot(sel);
    if (sel)
      sk[nsel + __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                          __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0))] = ru[jj];
    nsel += __popcll(m);
  }
  __builtin_amdgcn_wave_barrier();
  for (int r = lane; r < nsel; r += 64) {
    const unsigned long long kr = sk[r];
    int rank = 0;
    for (int j = 0; j < nsel; ++j) rank += sk[j] > kr ? 1 : 0;
    sel_k[rank] = static_cast<int>((0xFFFFFFFFu - static_cast<unsigned>(kr)) & KMASK);
  }
  return nsel;
}

// the inverse of beam_pack's score word (-0 comes back as +0)
__device__ __forceinline__ float beam_unpack_score(unsigned long long key) {
  const unsigned b = static_cast<unsigned>(key >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
}

// first stage of a selection over more candidates than one wave's registers hold: of the tot
// keys at ukey[0, tot) (lane l holds keys l, l + 64, ... in NJ registers) keep those that can
// be among the best `beam` of a superset -- the keys >= lb (lb as in beam_select: at least
// `beam` keys of the superset are >= it; 0 = none) if at most `beam` of them, else the best
// `beam` by beam_select's radix descent -- compacted into out[0, return value), unordered.
// The best `beam` of the superset are the best `beam` of the union of its parts' outputs.
template <int NJ>
__device__ __forceinline__ int beam_select_half(const unsigned long long* ukey, int tot, int beam,
                                                unsigned long long* out, int lane,
                                                unsigned long long lb) {
  unsigned long long ru[NJ];
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    const int k = lane + 64 * jj;
    ru[jj] = k < tot ? ukey[k] : 0ull;
  }
  auto count_ge = [&](unsigned long long c) {
    int n = 0;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) n += __popcll(__ballot(ru[jj] >= c));
    return n;
  };
  unsigned long long thr = lb != 0ull ? lb : 1ull;
  if (count_ge(thr) > beam) {
    unsigned long long t = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
      const unsigned long long c = t | (1ull << bit);
      const int n = count_ge(c);
      if (n >= beam) {
        t = c;
        if (n == beam) break;
      }
    }
    thr = t;   // the beam-th largest key or above it: exactly `beam` (unique) keys are >= thr
  }
  int nsel = 0;
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    const bool sel = ru[jj] >= thr;
    const unsigned long long m = __ballot(sel);
    if (sel)
      out[nsel + __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                           __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0))] = ru[jj];
    nsel += __popcll(m);
  }
  return nsel;
}

// Word n-gram LM of the beam search (ctcdecode's KenLM Scorer, decoder.py:90-99 with
// lm_path; tables built by ds2amd/lm.py from an ARPA file, oracle/ctc_beam_lm.py restates
// the semantics).  n-gram hash table: 32-byte records {w0..w5, log10 prob, log10 backoff}
// (ids -1 padded, w0 = -1 = empty slot), FNV-1a + avalanche, linear probing; vocabulary
// trie: dnext [S][C] arcs, dmask [S] the arcs as a char bit mask, dword [S] the word a
// state spells (-1 none); state 0 = start, fstate = after a word's space (no arcs).
struct BeamLm {
  int nstates;   // dict_states: an arc outside [0, nstates) leads to the post-space state (fstate)
  const int* dnext;
  const unsigned long long* dmask;
  const int* dword;
  const int4* tab;
  unsigned tmask;
  int fstate, order, start, space;
  double alpha, beta;
  // test hook (ds2_test_beam_stamps): per-phase shader-clock stamps (s_memtime) of
  // utterance 0's first BEAM_NSTAMP_T frames, [frame][phase], slot 8 = the frame start on
  // s_memrealtime (100 MHz); null = off
  unsigned long long* stamps;
};

constexpr int BEAM_NSTAMP_T = 256, BEAM_NSTAMP_P = 9;   // 8 phases + s_memrealtime
static unsigned long long* g_beam_stamps = nullptr;

constexpr int LM_MAX_ORDER = 6;

// The search over a stream (ds2_ctc_beam_stream_*): what survives from frame to frame, kept
// in global memory between launches.  Per stream one record of 32-bit words -- a header
// {BEAM_STREAM_MAGIC, beam_width, max_frames, entries in the beam, trie nodes in use, frames
// consumed, 0, 0}, then per-entry arrays of E = beam_width rounded up to 4 entries each: node,
// last char, pb, pnb, the node's parent, its best char log-prob, the prefix length, the LM's
// dictionary state and cached word score, and its LM_MAX_ORDER - 1 history words -- followed
// (after all records) by the trie arena of ds2_ctc_beam_decode's workspace layout, sized for
// max_frames frames.  The kernel only trusts a record whose header names the beam_width and
// max_frames it was launched with and whose counters fit the arena.
constexpr int BEAM_STREAM_MAGIC = 0x42534D31;
constexpr int BEAM_STREAM_HDR = 8;
constexpr int BEAM_STREAM_PER_ENTRY = 9 + (LM_MAX_ORDER - 1);
struct BeamStream {
  int* rec;            // [n][rec_words]
  int64_t rec_words;
  int* out_frames;     // [n] frames consumed so far per stream, or null
  int max_frames;
  int out_cap;         // row stride of out_ids / out_ts
};

__host__ __device__ inline int beam_stream_entries(int beam) { return (beam + 3) & ~3; }

__device__ __forceinline__ unsigned lm_hash(const int* k) {
  unsigned h = 2166136261u;
#pragma unroll
  for (int i = 0; i < LM_MAX_ORDER; ++i) h = (h ^ static_cast<unsigned>(k[i])) * 16777619u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  return h;
}

__device__ __forceinline__ bool lm_find(const BeamLm& L, const int* k, float& prob, float& bo) {
  unsigned s = lm_hash(k) & L.tmask;
  for (unsigned p = 0; p <= L.tmask; ++p) {
    const int4 a = L.tab[2 * s], b = L.tab[2 * s + 1];
    if (a.x == -1) return false;
    if (a.x == k[0] && a.y == k[1] && a.z == k[2] && a.w == k[3] && b.x == k[4] && b.y == k[5]) {
      prob = __int_as_float(b.z);
      bo = __int_as_float(b.w);
      return true;
    }
    s = (s + 1) & L.tmask;
  }
  return false;
}

// float(alpha * ln p(w | hist)) -- get_log_cond_prob(make_ngram(prefix)) * alpha; hist holds
// the order-1 preceding words, oldest first ("<s>" padded).  KenLM back-off: the longest
// n-gram ending in w gives the log10 prob, then the backoffs of every longer context
// suffix in the model are added (float32, shorter context first); an unknown word (w < 0:
// the partial word spells no vocabulary word) is OOV_SCORE = -1000.
__device__ __forceinline__ float lm_term(const BeamLm& L, const int* hist, int w) {
  const int n1 = L.order - 1;
  double lnp = -1000.0;
  if (w >= 0) {
    int key[LM_MAX_ORDER];
    float p = 0.f, bo = 0.f;
    int m = L.order;
    bool found = false;
    for (; m >= 1; --m) {
#pragma unroll
      for (int i = 0; i < LM_MAX_ORDER; ++i)
        key[i] = i < m - 1 ? hist[n1 - (m - 1) + i] : (i == m - 1 ? w : -1);
      if (lm_find(L, key, p, bo)) {
        found = true;
        break;
      }
    }
    if (found) {
      for (int ln = m; ln <= n1; ++ln) {
#pragma unroll
        for (int i = 0; i < LM_MAX_ORDER; ++i) key[i] = i < ln ? hist[n1 - ln + i] : -1;
        float pp, b;
        if (lm_find(L, key, pp, b)) p += b;
      }
      lnp = static_cast<double>(p) / static_cast<double>(0.4342944819f);   // NUM_FLT_LOGE
    }
  }
  return static_cast<float>(lnp * L.alpha);
}

// lm_term with every lookup's first probe issued at once: the order n-gram keys (n-gram
// orders order..1 ending in w) in one round of loads, then the back-off contexts (lengths
// m..order-1 of the history) in a second; a key whose first slot holds another key (a
// collision) continues with lm_find's linear probing from the next slot.  Same result as
// lm_term (same keys, same table, same float sums in the same order); two dependent rounds
// of table loads instead of up to 2 order - 1.
__device__ __forceinline__ bool lm_first_probe(const BeamLm& L, const int* k, int4& a, int4& b,
                                               unsigned& slot) {
  slot = lm_hash(k) & L.tmask;
  a = L.tab[2 * slot];
  b = L.tab[2 * slot + 1];
  return true;
}

__device__ __forceinline__ int lm_resolve(const BeamLm& L, const int* k, const int4& a,
                                          const int4& b, unsigned slot, float& prob, float& bo) {
  if (a.x == -1) return 0;
  if (a.x == k[0] && a.y == k[1] && a.z == k[2] && a.w == k[3] && b.x == k[4] && b.y == k[5]) {
    prob = __int_as_float(b.z);
    bo = __int_as_float(b.w);
    return 1;
  }
  // collision: probe on from the next slot (rare)
  unsigned sl = (slot + 1) & L.tmask;
  for (unsigned p = 1; p <= L.tmask; ++p) {
    const int4 c = L.tab[2 * sl], d = L.tab[2 * sl + 1];
    if (c.x == -1) return 0;
    if (c.x == k[0] && c.y == k[1] && c.z == k[2] && c.w == k[3] && d.x == k[4] && d.y == k[5]) {
      prob = __int_as_float(d.z);
      bo = __int_as_float(d.w);
      return 1;
    }
    sl = (sl + 1) & L.tmask;
  }
  return 0;
}

__device__ __forceinline__ float lm_term_par(const BeamLm& L, const int* hist, int w) {
  double lnp = -1000.0;
  if (w >= 0) {
    const int n1 = L.order - 1;
    int h[LM_MAX_ORDER - 1];
#pragma unroll
    for (int i = 0; i < LM_MAX_ORDER - 1; ++i) h[i] = i < n1 ? hist[i] : -1;
    // round 1: the n-grams of orders 1..order ending in w
    int4 ra[LM_MAX_ORDER], rb[LM_MAX_ORDER];
    unsigned rs[LM_MAX_ORDER];
#pragma unroll
    for (int m = 1; m <= LM_MAX_ORDER; ++m) {
      if (m > L.order) break;
      int key[LM_MAX_ORDER];
#pragma unroll
      for (int i = 0; i < LM_MAX_ORDER; ++i) key[i] = i < m - 1 ? h[n1 - (m - 1) + i] : (i == m - 1 ? w : -1);
      lm_first_probe(L, key, ra[m - 1], rb[m - 1], rs[m - 1]);
    }
    float p = 0.f, bo = 0.f;
    int m = L.order;
    bool found = false;
#pragma unroll
    for (int mm = LM_MAX_ORDER; mm >= 1; --mm) {
      if (mm > L.order || found) continue;
      int key[LM_MAX_ORDER];
#pragma unroll
      for (int i = 0; i < LM_MAX_ORDER; ++i) key[i] = i < mm - 1 ? h[n1 - (mm - 1) + i] : (i == mm - 1 ? w : -1);
      if (lm_resolve(L, key, ra[mm - 1], rb[mm - 1], rs[mm - 1], p, bo)) {
        found = true;
        m = mm;
      }
    }
    if (found) {
      // round 2: the back-offs of the contexts of lengths m..order-1
      int4 ca[LM_MAX_ORDER - 1], cb[LM_MAX_ORDER - 1];
      unsigned cs[LM_MAX_ORDER - 1];
#pragma unroll
      for (int ln = 1; ln < LM_MAX_ORDER; ++ln) {
        if (ln < m || ln > n1) continue;
        int key[LM_MAX_ORDER];
#pragma unroll
        for (int i = 0; i < LM_MAX_ORDER; ++i) key[i] = i < ln ? h[n1 - ln + i] : -1;
        lm_first_probe(L, key, ca[ln - 1], cb[ln - 1], cs[ln - 1]);
      }
#pragma unroll
      for (int ln = 1; ln < LM_MAX_ORDER; ++ln) {
        if (ln < m || ln > n1) continue;
        int key[LM_MAX_ORDER];
#pragma unroll
        for (int i = 0; i < LM_MAX_ORDER; ++i) key[i] = i < ln ? h[n1 - ln + i] : -1;
        float pp, b2;
        if (lm_resolve(L, key, ca[ln - 1], cb[ln - 1], cs[ln - 1], pp, b2)) p += b2;
      }
      lnp = static_cast<double>(p) / static_cast<double>(0.4342944819f);   // NUM_FLT_LOGE
    }
  }
  return static_cast<float>(lnp * L.alpha);
}

// log_p += score; log_p += beta (float, then a double add rounded to float)
__device__ __forceinline__ float lm_add(float v, float term, double beta) {
  return static_cast<float>(static_cast<double>(v + term) + beta);
}

// wave minimum (every lane gets it)
// alive child of trie node p with char c, or -1 (the lists only grow; dead nodes stay)
__device__ int trie_alive_child(const int* fc, const int* ns, const int* chr, const int* cnt,
                                int p, int c, int64_t cap) {
  int x = __hip_atomic_load(fc + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int64_t g = 0; x > 0 && g < cap; ++g) {
    if (chr[x] == c && __hip_atomic_load(cnt + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0)
      return x;
    x = ns[x];
  }
  return -1;
}

// wave minimum in VALU only (DPP: quad permutes, half-row and row mirrors, row_bcast:15 and
// :31 -- lane 63 ends with the minimum), no LDS round trip; every lane gets it
template <int CTRL, int RMASK>
__device__ __forceinline__ float dpp_min_step(float x) {
  const int y = __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x),
                                            CTRL, RMASK, 0xf, false);
  return fminf(x, __builtin_bit_cast(float, y));
}
__device__ __forceinline__ float wave_min_dpp(float v) {
  v = dpp_min_step<0xB1, 0xf>(v);    // quad_perm [1, 0, 3, 2]
  v = dpp_min_step<0x4E, 0xf>(v);    // quad_perm [2, 3, 0, 1]
  v = dpp_min_step<0x141, 0xf>(v);   // row_half_mirror
  v = dpp_min_step<0x140, 0xf>(v);   // row_mirror
  v = dpp_min_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1, 3
  v = dpp_min_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// STREAM = true is the same search over one chunk of a stream: the beam comes from the
// stream's record (BeamStream) instead of the root seed, char frames are counted from the
// frames the stream consumed before, and the beam goes back to the record after the chunk;
// the ranking and back-tracking run only where the caller passed outputs, and leave the
// record alone.
template <int BM, int CM, bool LM, bool STREAM = false>
__global__ __launch_bounds__(64) void ctc_beam_kernel(
    const float* __restrict__ probs, int t_max, int C, int64_t stride_n, int64_t stride_t,
    const int* __restrict__ sizes, int blank, int beam, int cutoff_top_n, double cutoff_prob,
    int top_paths, int* __restrict__ node_parent, int* __restrict__ node_ch,
    int* __restrict__ node_ts, float* __restrict__ node_lpc, int* __restrict__ node_cnt,
    int* __restrict__ node_fc, int* __restrict__ node_ns, unsigned long long* __restrict__ node_km,
    int64_t node_cap, int* __restrict__ out_ids, int* __restrict__ out_ts, int* __restrict__ out_lens,
    float* __restrict__ out_scores, BeamLm L, BeamStream S) {
  constexpr int EPL = (BM + 63) / 64;   // beam entries per lane
  // more candidates than 12 key bits and one wave's registers hold (the wide instantiation)
  constexpr bool WIDE = BM * CM > 4096;
  static_assert(BM * CM <= 8192 && CM <= 64, "candidate index: 13 bits, char + 1: 7 bits");
  constexpr int KSTRIDE = WIDE ? 8192 : 4096;          // key = (char + 1) * KSTRIDE + k
  constexpr unsigned KMASK = KSTRIDE - 1;
  constexpr int TCH = WIDE ? BEAM_WIDE_TCH : BEAM_TCH;   // frames staged at a time
  using rl_t = std::conditional_t<WIDE, unsigned short, int>;   // a candidate index
  // LM state per beam entry: trie state, the order-1 preceding words, the cached
  // alpha-scaled LM score of the entry's current word (used by a space extension and by
  // the final scoring); per frame the char an entry's dictionary reset consumes and its
  // valid-extension mask
  constexpr int LB = LM ? BM : 1;
  __shared__ int b_dst[2][LB];
  __shared__ int b_hist[2][LB][LM_MAX_ORDER - 1];
  __shared__ float b_lms[2][LB];
  __shared__ int cstar[LB];
  __shared__ unsigned long long vmask[LB];
  __shared__ float lp[CM];
  __shared__ int allowed[CM];
  __shared__ int order[CM];
  __shared__ int b_node[2][BM], b_last[2][BM];
  __shared__ float b_pb[2][BM], b_pnb[2][BM];
  // per-entry copies of the entry's trie node's parent and best last-char log-prob, so
  // the per-frame chain has no global-memory reads (the trie is written, never read,
  // until the final back-tracking)
  __shared__ int b_par[2][BM];
  __shared__ float b_lpc[2][BM];
  __shared__ int b_len[2][BM];   // prefix length (the node's depth): one back-tracking walk
  __shared__ float score[BM];
  __shared__ unsigned long long cmask[BM];   // chars of the entry's in-beam children
  // every candidate's pb / pnb; the wide instantiation has no room for them and rebuilds a
  // winner's pair: a blank candidate's is its entry's bl_pb / bl_pnb, an extension's is
  // (-inf, its score), the score being the key's high word
  constexpr int NCP = WIDE ? 1 : BM * CM;
  __shared__ float cpb[NCP], cpnb[NCP];
  __shared__ unsigned long long ukey[BM * CM];   // beam_pack(score, key) per candidate k
  __shared__ unsigned long long sk_sel[BM > 64 ? BM : 64];   // the selected keys (beam_select)
  __shared__ unsigned long long sk_half[WIDE ? 2 * BM : 1];  // the two halves' (beam_select_half)
  __shared__ float bl_sc[BM], bl_pb[BM], bl_pnb[BM];   // the blank candidate of each entry
  __shared__ int sel_k[BM];
  __shared__ int s_nb, s_nodes, s_nr;
  // trie revival: per entry its node's alive-children chars; the attempted extensions onto
  // pruned-but-alive children (their char frames are updated after the scoring loop); the
  // entries of the old beam that stay
  __shared__ unsigned long long b_km[BM];
  __shared__ rl_t rlist[BM * CM];
  __shared__ int kept[BM];
  __shared__ float pch[TCH * CM];
  static_assert(sizeof(b_dst) + sizeof(b_hist) + sizeof(b_lms) + sizeof(cstar) + sizeof(vmask) +
                    sizeof(lp) + sizeof(allowed) + sizeof(order) + sizeof(b_node) +
                    sizeof(b_last) + sizeof(b_pb) + sizeof(b_pnb) + sizeof(b_par) +
                    sizeof(b_lpc) + sizeof(b_len) + sizeof(score) + sizeof(cmask) + sizeof(cpb) +
                    sizeof(cpnb) + sizeof(ukey) + sizeof(sk_sel) + sizeof(sk_half) +
                    sizeof(bl_sc) + sizeof(bl_pb) + sizeof(bl_pnb) + sizeof(sel_k) +
                    3 * sizeof(int) + sizeof(b_km) + sizeof(rlist) + sizeof(kept) + sizeof(pch) <=
                    BEAM_LDS_PER_CU,
                "ctc_beam_kernel: static LDS over the budget (a CU has 160 KiB)");

  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  int size = sizes != nullptr ? sizes[n] : t_max;
  size = size < 0 ? 0 : (size > t_max ? t_max : size);
  const float* pn = probs + (int64_t)n * stride_n;
  int* par = node_parent + (int64_t)n * node_cap;
  int* chr = node_ch + (int64_t)n * node_cap;
  int* tst = node_ts + (int64_t)n * node_cap;
  float* lpcv = node_lpc + (int64_t)n * node_cap;
  int* cnt = node_cnt + (int64_t)n * node_cap;
  int* fc = node_fc + (int64_t)n * node_cap;
  int* ns = node_ns + (int64_t)n * node_cap;
  unsigned long long* km = node_km + (int64_t)n * node_cap;
  const bool prune = cutoff_prob < 1.0 || cutoff_top_n < C;
  unsigned long long* const stamps = (L.stamps != nullptr && n == 0) ? L.stamps : nullptr;
#define BEAM_STAMP(ph)                                                      \
  if (stamps != nullptr && t < BEAM_NSTAMP_T && lane == 0)                  \
    stamps[t * BEAM_NSTAMP_P + (ph)] = __builtin_amdgcn_s_memtime();

  int t0 = 0;   // frames this stream consumed in earlier launches
  int* rec = nullptr;
  [[maybe_unused]] int rec_e = 0;
  [[maybe_unused]] bool rec_ok = false;
  if constexpr (STREAM) {
    rec = S.rec + (int64_t)n * S.rec_words;
    rec_e = beam_stream_entries(beam);
    const int h_nb = rec[3], h_nodes = rec[4], h_t0 = rec[5];
    rec_ok = rec[0] == BEAM_STREAM_MAGIC && rec[1] == beam && rec[2] == S.max_frames &&
             h_nb >= 0 && h_nb <= beam && h_t0 >= 0 && h_t0 <= S.max_frames && h_nodes >= 1 &&
             (int64_t)h_nodes <= (int64_t)h_t0 * beam + 1 &&
             (int64_t)S.max_frames * beam + 1 <= node_cap;
    // every frame adds at most `beam` nodes: within max_frames frames the arena holds them
    t0 = rec_ok ? h_t0 : 0;
    size = rec_ok ? min(size, S.max_frames - t0) : 0;
    const int nb0 = rec_ok ? h_nb : 0;
    const int* re = rec + BEAM_STREAM_HDR;
    for (int e = lane; e < nb0; e += 64) {
      b_node[0][e] = re[e];
      b_last[0][e] = re[rec_e + e];
      b_pb[0][e] = __int_as_float(re[2 * rec_e + e]);
      b_pnb[0][e] = __int_as_float(re[3 * rec_e + e]);
      b_par[0][e] = re[4 * rec_e + e];
      b_lpc[0][e] = __int_as_float(re[5 * rec_e + e]);
      b_len[0][e] = re[6 * rec_e + e];
      if constexpr (LM) {
        b_dst[0][e] = re[7 * rec_e + e];
        b_lms[0][e] = __int_as_float(re[8 * rec_e + e]);
        // the root's history is "<s>" throughout, whichever LM the stream is fed with (the
        // initialiser does not know it)
        for (int h = 0; h < LM_MAX_ORDER - 1; ++h)
          b_hist[0][e][h] = re[e] == 0 ? L.start : re[9 * rec_e + e * (LM_MAX_ORDER - 1) + h];
      }
    }
    if (lane == 0) {
      s_nb = nb0;
      s_nodes = rec_ok ? h_nodes : 1;
    }
  } else if (lane == 0) {
    b_node[0][0] = 0; b_last[0][0] = -1; b_pb[0][0] = 0.f; b_pnb[0][0] = -INFINITY;
    b_par[0][0] = -1; b_lpc[0][0] = -INFINITY; b_len[0][0] = 0;
    par[0] = -1; chr[0] = -1; tst[0] = -1; lpcv[0] = -INFINITY;
    cnt[0] = 1; fc[0] = -1; ns[0] = -1; km[0] = 0ull;
    s_nb = 1;
    s_nodes = 1;
    if constexpr (LM) {
      b_dst[0][0] = 0;
      for (int h = 0; h < LM_MAX_ORDER - 1; ++h) b_hist[0][0][h] = L.start;
      b_lms[0][0] = 0.f;
    }
  }
  __syncthreads();
  int cur = 0;
  unsigned long long km_next[EPL];   // children masks of the beam's entries' nodes (prefetched)
#pragma unroll
  for (int q = 0; q < EPL; ++q) km_next[q] = 0ull;   // the root starts childless
  if constexpr (STREAM) {
#pragma unroll
    for (int q = 0; q < EPL; ++q) {
      const int e = lane + 64 * q;
      if (e < s_nb)
        km_next[q] = __hip_atomic_load(km + b_node[0][e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (int t = 0; t < size; ++t) {
    const int nb = s_nb;
    if (nb == 0) break;
    BEAM_STAMP(0)
    if (stamps != nullptr && t < BEAM_NSTAMP_T && lane == 0)
      stamps[t * BEAM_NSTAMP_P + 8] = __builtin_amdgcn_s_memrealtime();
    const int tc = t % TCH;
    if (tc == 0) {   // stage the next TCH frames (all loads of a lane in flight at once)
      const int nf = min(TCH, size - t);
#pragma unroll 8
      for (int e = lane; e < TCH * C; e += 64) {
        const int f = e / C;
        const int c = e - f * C;
        pch[f * CM + c] = f < nf ? pn[(int64_t)(t + f) * stride_t + c] : 0.f;
      }
      __syncthreads();
    }
    const float* pf = pch + tc * CM;
    // ---- vocabulary pruning and log probs
    float pv = 0.f;
    if (lane < C) {
      pv = pf[lane];
      // ctcdecode's get_pruned_log_probs: log of the double prob + FLT_MIN, stored as float
      lp[lane] = static_cast<float>(log(static_cast<double>(pv) + 1.1754943508222875e-38));
    }
    if (prune) {
      // rank of this lane's probability: C uniform lane reads (v_readlane), no LDS
      int rank = 0;
#pragma unroll
      for (int k = 0; k < CM; ++k) {
        if (CM > 32 && k >= C) break;
        const float q = __builtin_bit_cast(
            float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pv), k));
        rank += (k < C && (q > pv || (q == pv && k < lane))) ? 1 : 0;
      }
      if (lane < C) order[rank] = lane;
      __syncthreads();
      if (lane < C) {
        int ok = rank < cutoff_top_n;
        if (ok && cutoff_prob < 1.0) {
          double cum = 0.0;
          for (int r = 0; r < rank; ++r) cum += (double)pf[order[r]];
          ok = cum < cutoff_prob;
        }
        allowed[lane] = ok;
      }
    } else if (lane < C) {
      allowed[lane] = 1;
    }
    BEAM_STAMP(1)
    // ---- beam bookkeeping, one pass per entry (lane e) over data the previous frame left in
    // LDS, with no barrier inside: its score, its parent's index in the beam (jp), the chars
    // of its node's children that are themselves in the beam (cmask: an extension onto one of
    // them merges into that entry instead), the LM bound and masks, and its blank candidate
    // ("stay" terms plus the merge of the parent's extension by the entry's last char; the
    // parent's score recomputed here rather than read after a barrier)
    if (lane == 0) s_nr = 0;
    float cut = -INFINITY;   // LM: min_cutoff once the beam is full, else -inf; wave-uniform
    float blmin = INFINITY;  // the worst blank-candidate score of the beam (wave-uniform)
    {
      float sce[EPL];
      int jpe[EPL];
      // every entry's (node, parent, last char) in registers (lane l: entry l + 64 r), so the
      // scan over the beam below is v_readlane + VALU, not a chain of LDS round trips
      int bnr[EPL], bpr[EPL], blr[EPL];
#pragma unroll
      for (int r = 0; r < EPL; ++r) {
        const int e = lane + 64 * r;
        const bool in = e < nb;
        bnr[r] = in ? b_node[cur][e] : -2;
        bpr[r] = in ? b_par[cur][e] : -2;
        blr[r] = in ? b_last[cur][e] : 0;
      }
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        const int e = lane + 64 * q;
        sce[q] = INFINITY;
        const int nd = bnr[q];
        const int pnode = nd > 0 ? bpr[q] : -1;
        int j = -1;
        unsigned long long cm = 0ull;
#pragma unroll
        for (int r = 0; r < EPL; ++r) {
          const int lim = min(64, nb - 64 * r);          // wave-uniform
          for (int l = 0; l < lim; ++l) {
            const int ni = __builtin_amdgcn_readlane(bnr[r], l);
            const int pi = __builtin_amdgcn_readlane(bpr[r], l);
            const int li = __builtin_amdgcn_readlane(blr[r], l);
            if (pnode >= 0 && ni == pnode) j = 64 * r + l;
            if (ni > 0 && pi == nd) cm |= 1ull << li;
          }
        }
        jpe[q] = -1;
        if (e < nb) {
          const float sc = beam_lse(b_pb[cur][e], b_pnb[cur][e]);
          score[e] = sc;
          sce[q] = sc;
          b_km[e] = km_next[q];
          kept[e] = 0;
          jpe[q] = j;
          cmask[e] = cm;
        }
      }
      // ---- LM: the scorer's pruning bound (min_cutoff = worst beam score + log p_blank -
      // max(0, beta), applied once the beam is full), the dictionary reset of post-space
      // entries (their first attempted non-blank char is rejected and the trie state goes
      // back to the start) and each entry's valid-extension mask
      if constexpr (LM) {
        float wv = INFINITY;
#pragma unroll
        for (int q = 0; q < EPL; ++q) wv = fminf(wv, sce[q]);
        wv = wave_min(wv);
        const double pbl = static_cast<double>(pf[blank]);
        const float mincut = static_cast<float>(
            static_cast<double>(wv) + (pbl > 0.0 ? log(pbl) : -INFINITY) - fmax(0.0, L.beta));
        cut = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(
                                            int, nb == beam ? mincut : -INFINITY)));
#pragma unroll
        for (int q = 0; q < EPL; ++q) {
          const int e = lane + 64 * q;
          if (e < nb) {
            const int s = b_dst[cur][e];
            int cs = -1;
            unsigned long long vm;
            if (s == L.fstate) {
              const float se = sce[q];
              for (int r = 0; r < C; ++r) {
                const int cc = prune ? order[r] : r;
                if (cc == blank || !allowed[cc]) continue;
                if (!(lp[cc] + se < cut)) {
                  cs = cc;
                  break;
                }
              }
              vm = L.dmask[0] & ~(cs >= 0 ? (1ull << cs) : 0ull);
            } else {
              vm = L.dmask[s];
            }
            cstar[e] = cs;
            vmask[e] = vm;
          }
        }
      }
      // ---- the blank candidate of every entry
      float blsr[EPL];
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        blsr[q] = INFINITY;
        const int i = lane + 64 * q;
        if (i < nb) {
          const int last_i = blr[q];
          const float sc_i = sce[q];
          // with an LM a (prefix, char) pair below the pruning bound is skipped entirely
          const float pb = (allowed[blank] && !(lp[blank] + sc_i < cut)) ? lp[blank] + sc_i : -INFINITY;
          float pnb = (last_i >= 0 && allowed[last_i] && !(lp[last_i] + sc_i < cut))
                          ? lp[last_i] + b_pnb[cur][i] : -INFINITY;
          const int jp = jpe[q];
          if (jp >= 0) {
            const float pb_jp = b_pb[cur][jp];
            const float sc_jp = beam_lse(pb_jp, b_pnb[cur][jp]);
            if (allowed[last_i] && !(lp[last_i] + sc_jp < cut)) {
              float e = (last_i == b_last[cur][jp])
                            ? (pb_jp != -INFINITY ? lp[last_i] + pb_jp : -INFINITY)
                            : lp[last_i] + sc_jp;
              if (LM && last_i == L.space) e = lm_add(e, b_lms[cur][jp], L.beta);
              pnb = beam_lse(pnb, e);
              const int nd = bnr[q];
              if (lp[last_i] > b_lpc[cur][i]) {
                b_lpc[cur][i] = lp[last_i];
                lpcv[nd] = lp[last_i];
                tst[nd] = t0 + t;
              }
            }
          }
          bl_pb[i] = pb;
          bl_pnb[i] = pnb;
          const float bs = beam_lse(pb, pnb);
          bl_sc[i] = bs;
          blsr[q] = bs;
        }
      }
      float bm = INFINITY;
#pragma unroll
      for (int r = 0; r < EPL; ++r) bm = fminf(bm, blsr[r]);
      blmin = wave_min_dpp(bm);
    }
    __syncthreads();
    BEAM_STAMP(2)
    // ---- candidates k = i * C + c: lane (g, c) = divmod(lane, CW) scores char c of the entries
    // i = G jj + g, so the char's log prob and pruning flag stay in registers and every
    // per-entry read is one LDS address per lane group (a broadcast).  Entries go in groups of
    // SG: every LDS read of a group is issued before any of its arithmetic, which is
    // branch-free (the blank lane takes its entry's precomputed blank candidate); packed keys
    // go to ukey[k] for the selection
    {
      // lane groups of 32 when the vocabulary fits (the small instantiation's CM = 64 would
      // leave half the wave idle on the model's 29 labels): G entries per pass
      constexpr int SG = 4;
      const int CW = (CM > 32 && C <= 32) ? 32 : CM;     // wave-uniform
      const int G = 64 / CW;
      const int c = lane & (CW - 1), g = lane / CW;
      const bool cv = c < C;
      const int cs = cv ? c : 0;                          // an in-range char for idle lanes
      const float lpc = lp[cs];
      const bool alc = cv && c != blank && allowed[cs];
      const bool isb = c == blank;
      const int jn = (nb + G - 1) / G;                  // wave-uniform
      for (int j0 = 0; j0 < jn; j0 += SG) {
        int last[SG];
        float sci[SG], pbi[SG], blp[SG], blnp[SG], bls[SG], lms[SG];
        unsigned long long kmi[SG], vmi[SG], cmi[SG];
#pragma unroll
        for (int u = 0; u < SG; ++u) {
          const int ir = G * (j0 + u) + g;
          const int i = ir < BM ? ir : BM - 1;            // in-bounds reads; validity below
          last[u] = b_last[cur][i];
          sci[u] = score[i];
          pbi[u] = b_pb[cur][i];
          cmi[u] = cmask[i];
          kmi[u] = b_km[i];
          blp[u] = bl_pb[i];
          blnp[u] = bl_pnb[i];
          bls[u] = bl_sc[i];
          if constexpr (LM) {
            vmi[u] = vmask[i];
            lms[u] = b_lms[cur][i];
          } else {
            vmi[u] = 0ull;
            lms[u] = 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < SG; ++u) {
          const int i = G * (j0 + u) + g;
          const int k = i * C + c;
          // with an LM a (prefix, char) pair below the pruning bound is skipped entirely
          const bool ext = alc && !((cmi[u] >> cs) & 1ull) &&
                           (!LM || (!(lpc + sci[u] < cut) && ((vmi[u] >> cs) & 1ull)));
          float pe = (c == last[u]) ? (pbi[u] != -INFINITY ? lpc + pbi[u] : -INFINITY)
                                    : lpc + sci[u];
          if constexpr (LM) pe = c == L.space ? lm_add(pe, lms[u], L.beta) : pe;
          const float pb = isb ? blp[u] : -INFINITY;
          const float pnb = isb ? blnp[u] : (ext ? pe : -INFINITY);
          const float sc = isb ? bls[u] : (ext ? pe : -INFINITY);
          if (cv && i < nb) {
            if constexpr (!WIDE) {
              cpb[k] = pb;
              cpnb[k] = pnb;
            }
            ukey[k] = beam_pack(sc, ((isb ? last[u] : c) + 1) * KSTRIDE + k);
            if (ext && ((kmi[u] >> c) & 1ull))
              rlist[atomicAdd(&s_nr, 1)] = static_cast<rl_t>(k);   // revival attempt
          }
        }
      }
    }
    __syncthreads();
    BEAM_STAMP(3)
    // ---- attempted extensions onto pruned-but-alive trie nodes take the log_prob_c rule
    // (get_path_trie updates a found child whether or not it is kept)
    for (int r = lane; r < s_nr; r += 64) {
      const int k = rlist[r];
      const int i = k / C, c = k - (k / C) * C;
      const int x = trie_alive_child(fc, ns, chr, cnt, b_node[cur][i], c, node_cap);
      if (x > 0 && lp[c] > lpcv[x]) {
        lpcv[x] = lp[c];
        tst[x] = t0 + t;
      }
    }
    BEAM_STAMP(4)
    // ---- keep the best `beam` candidates (beam_select, its registers sized to the filled slots)
    constexpr int SD = BM * CM / 64;
    const int tot = nb * C;
    const int jd = (tot + 63) / 64;
    // a lower bound of the selection: the score word of the worst of the nb >= beam blank
    // candidates with an empty key word (they are real candidates, so at least `beam` keys are
    // >= it); 0 (none) while the beam is not full or some entry has no blank candidate
    const unsigned long long lb = (nb >= beam && blmin > -INFINITY)
                                      ? (beam_pack(blmin, 0) & 0xFFFFFFFF00000000ull) : 0ull;
    int nsel;
    if constexpr (!WIDE) {
      nsel = jd <= 2    ? beam_select<2>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 4  ? beam_select<4>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 6  ? beam_select<6>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 8  ? beam_select<8>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 16 ? beam_select<16>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
                        : beam_select<SD>(ukey, tot, beam, sel_k, sk_sel, lane, lb);
    } else if (jd <= SD / 2) {
      // up to 4096 candidates (100 entries x 36 labels are 3600): one selection, as above
      nsel = jd <= 2    ? beam_select<2, KMASK>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 4  ? beam_select<4, KMASK>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 8  ? beam_select<8, KMASK>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 16 ? beam_select<16, KMASK>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
             : jd <= 32 ? beam_select<32, KMASK>(ukey, tot, beam, sel_k, sk_sel, lane, lb)
                        : beam_select<SD / 2, KMASK>(ukey, tot, beam, sel_k, sk_sel, lane, lb);
    } else {
      // more: SD keys per lane are twice the registers.  Each half of the candidates gives up
      // its best `beam` (or just its keys >= lb when those are fewer), and the best `beam` of
      // the two lists -- which hold the best `beam` of all -- are selected and ranked
      constexpr int HALF = 64 * (SD / 2);
      const int n0 = beam_select_half<SD / 2>(ukey, HALF, beam, sk_half, lane, lb);
      const int n1 = beam_select_half<SD / 2>(ukey + HALF, tot - HALF, beam, sk_half + n0, lane, lb);
      __syncthreads();
      nsel = beam_select<2 * BM / 64, KMASK>(sk_half, n0 + n1, beam, sel_k, sk_sel, lane, lb);
    }
    __syncthreads();
    BEAM_STAMP(5)
    // ---- new beam: lane r builds entries r, r + 64, ...; new prefixes get trie nodes in
    // rank order (node = first free + the number of extensions ranked before it)
    const int nxt = cur ^ 1;
    {
      const int nodes0 = s_nodes;
      int run = 0;
      // a new node's sibling link (the parent's previous first child, returned by the
      // exchange) is stored after the deaths below, so no lane waits for the exchange here
      int ns_node[EPL], ns_val[EPL];
      // revived nodes first: every lookup reads only the trie as the previous frame left it
      int rv[EPL];
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        const int e = lane + 64 * q;
        rv[q] = -1;
        if (e < nsel) {
          const int k = sel_k[e];
          const int i = k / C, c = k - (k / C) * C;
          if (c != blank && ((b_km[i] >> c) & 1ull))
            rv[q] = trie_alive_child(fc, ns, chr, cnt, b_node[cur][i], c, node_cap);
        }
      }
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        const int e = lane + 64 * q;
        ns_node[q] = -1;
        int k = 0, i = 0, c = blank;
        if (e < nsel) {
          k = sel_k[e];
          i = k / C;
          c = k - i * C;
        }
        const bool ext = e < nsel && c != blank;
        const bool revived = ext && rv[q] > 0;
        const unsigned long long em = __ballot(ext && !revived);
        const int before = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(em >> 32),
                                                     __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(em), 0));
        if (e < nsel) {
          if constexpr (LM) {
            const int n1 = L.order - 1;
            int si = b_dst[cur][i];
            if (!ext) {
              // the dictionary reset sticks to the node
              b_dst[nxt][e] = (si == L.fstate && cstar[i] >= 0) ? 0 : si;
              for (int h = 0; h < n1; ++h) b_hist[nxt][e][h] = b_hist[cur][i][h];
              b_lms[nxt][e] = b_lms[cur][i];
            } else {
              if (si == L.fstate) si = 0;
              if (c == L.space) {   // the space completes the word of state si
                // (a revived post-space node has a child: its reset has happened)
                b_dst[nxt][e] = revived ? 0 : L.fstate;
                for (int h = 0; h + 1 < n1; ++h) b_hist[nxt][e][h] = b_hist[cur][i][h + 1];
                if (n1 > 0) b_hist[nxt][e][n1 - 1] = L.dword[si];
                b_lms[nxt][e] = 0.f;
              } else {
                int ns = L.dnext[(int64_t)si * C + c];
                if ((unsigned)ns >= (unsigned)L.nstates) ns = L.fstate;   // a malformed arc
                b_dst[nxt][e] = ns;
                for (int h = 0; h < n1; ++h) b_hist[nxt][e][h] = b_hist[cur][i][h];
                b_lms[nxt][e] = lm_term_par(L, &b_hist[cur][i][0], L.dword[ns]);
              }
            }
          }
          if (!ext) {
            b_node[nxt][e] = b_node[cur][i];
            b_last[nxt][e] = b_last[cur][i];
            b_par[nxt][e] = b_par[cur][i];
            b_lpc[nxt][e] = b_lpc[cur][i];
            b_len[nxt][e] = b_len[cur][i];
            kept[i] = 1;
          } else if (revived) {
            const int x = rv[q];
            atomicAdd(cnt + x, 1);
            b_node[nxt][e] = x;
            b_last[nxt][e] = c;
            b_par[nxt][e] = b_node[cur][i];
            b_lpc[nxt][e] = lpcv[x];
            b_len[nxt][e] = b_len[cur][i] + 1;
          } else {
            const int nd = nodes0 + run + before;
            const int p = b_node[cur][i];
            par[nd] = p;
            chr[nd] = c;
            tst[nd] = t0 + t;
            lpcv[nd] = lp[c];
            cnt[nd] = 1;
            fc[nd] = -1;
            km[nd] = 0ull;
            ns_node[q] = nd;
            ns_val[q] = atomicExch(fc + p, nd);
            atomicAdd(cnt + p, 1);
            atomicOr(km + p, 1ull << c);
            b_node[nxt][e] = nd;
            b_last[nxt][e] = c;
            b_par[nxt][e] = b_node[cur][i];
            b_lpc[nxt][e] = lp[c];
            b_len[nxt][e] = b_len[cur][i] + 1;
          }
          if constexpr (!WIDE) {
            b_pb[nxt][e] = cpb[k];
            b_pnb[nxt][e] = cpnb[k];
          } else {
            b_pb[nxt][e] = ext ? -INFINITY : bl_pb[i];
            b_pnb[nxt][e] = ext ? beam_unpack_score(ukey[k]) : bl_pnb[i];
          }
        }
        run += __popcll(em);
      }
      __syncthreads();
      BEAM_STAMP(6)
      // pruned entries leave the beam; a node with no alive child left dies and takes its
      // bit and count out of its parent (recursively; the root never dies)
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        const int e = lane + 64 * q;
        if (e < nb && !kept[e]) {
          int x = b_node[cur][e];
          for (int64_t g = 0; x > 0 && g < node_cap; ++g) {
            if (atomicSub(cnt + x, 1) != 1) break;
            const int p = par[x];
            atomicAnd(km + p, ~(1ull << chr[x]));
            x = p;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < EPL; ++q)
        if (ns_node[q] >= 0) ns[ns_node[q]] = ns_val[q];
      if (lane == 0) {
        s_nodes = nodes0 + run;
        s_nb = nsel;
      }
      // the next frame's children masks, loaded now (after this frame's trie updates, in
      // issue order) and consumed by its bookkeeping
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        const int e = lane + 64 * q;
        if (e < nsel)
          km_next[q] = __hip_atomic_load(km + b_node[nxt][e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    BEAM_STAMP(7)
    cur = nxt;
  }
#undef BEAM_STAMP
  const int nb = s_nb;
  if constexpr (STREAM) {
    // the beam goes back to its record (a chunk without valid frames leaves it as it is)
    if (rec_ok && size > 0) {
      int* re = rec + BEAM_STREAM_HDR;
      for (int e = lane; e < nb; e += 64) {
        re[e] = b_node[cur][e];
        re[rec_e + e] = b_last[cur][e];
        re[2 * rec_e + e] = __float_as_int(b_pb[cur][e]);
        re[3 * rec_e + e] = __float_as_int(b_pnb[cur][e]);
        re[4 * rec_e + e] = b_par[cur][e];
        re[5 * rec_e + e] = __float_as_int(b_lpc[cur][e]);
        re[6 * rec_e + e] = b_len[cur][e];
        if constexpr (LM) {
          re[7 * rec_e + e] = b_dst[cur][e];
          re[8 * rec_e + e] = __float_as_int(b_lms[cur][e]);
          for (int h = 0; h < LM_MAX_ORDER - 1; ++h)
            re[9 * rec_e + e * (LM_MAX_ORDER - 1) + h] = b_hist[cur][e][h];
        }
      }
      if (lane == 0) {
        rec[3] = nb;
        rec[4] = s_nodes;
        rec[5] = t0 + size;
      }
    }
    if (lane == 0 && S.out_frames != nullptr) S.out_frames[n] = rec_ok ? t0 + size : -1;
    if (out_lens == nullptr) return;   // no read-out asked for
  }
  // ---- final ranking and back-tracking (one lane per returned path)
  const int ocap = STREAM ? S.out_cap : t_max;   // row stride of out_ids / out_ts
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int e = lane + 64 * q;
    if (e < nb) {
      float s = beam_lse(b_pb[cur][e], b_pnb[cur][e]);
      // LM: the last word of every non-empty prefix not ending in a space is scored too
      if (LM && b_node[cur][e] != 0 && b_last[cur][e] != L.space)
        s = s + static_cast<float>(static_cast<double>(b_lms[cur][e]) + L.beta);
      score[e] = s;
    }
  }
  __syncthreads();
  for (int e = lane; e < nb; e += 64) {
    int rank = 0;
    const float s0 = score[e];
    const int key0 = (b_last[cur][e] + 1) * 4096 + e;
    for (int i = 0; i < nb; ++i)
      if (i != e && beam_better(score[i], (b_last[cur][i] + 1) * 4096 + i, s0, key0)) ++rank;
    if (rank < top_paths) {
      const int len = b_len[cur][e];
      int* ids = out_ids + ((int64_t)n * top_paths + rank) * ocap;
      int* tsp = out_ts + ((int64_t)n * top_paths + rank) * ocap;
      int pos = len;
      for (int nd = b_node[cur][e]; nd > 0 && pos > 0; nd = par[nd]) {
        --pos;
        if (STREAM && pos >= ocap) continue;   // a caller whose out_cap understates its feeds
        ids[pos] = chr[nd];
        tsp[pos] = tst[nd];
      }
      out_lens[n * top_paths + rank] = len;
      out_scores[n * top_paths + rank] = s0;
    }
  }
  for (int r = nb + lane; r < top_paths; r += 64) {   // fewer prefixes than paths asked for
    out_lens[n * top_paths + r] = 0;
    out_scores[n * top_paths + r] = -INFINITY;
  }
}

// a stream's record and trie as the whole-utterance kernel seeds them: the root-only beam
__global__ __launch_bounds__(64) void ctc_beam_stream_init_kernel(
    int* __restrict__ rec_all, int64_t rec_words, int beam, int max_frames,
    int* __restrict__ node_parent, int* __restrict__ node_ch, int* __restrict__ node_ts,
    float* __restrict__ node_lpc, int* __restrict__ node_cnt, int* __restrict__ node_fc,
    int* __restrict__ node_ns, unsigned long long* __restrict__ node_km, int64_t node_cap) {
  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  int* rec = rec_all + (int64_t)n * rec_words;
  for (int64_t i = lane; i < rec_words; i += 64) rec[i] = 0;
  __syncthreads();
  if (lane == 0) {
    const int E = beam_stream_entries(beam);
    int* re = rec + BEAM_STREAM_HDR;
    rec[0] = BEAM_STREAM_MAGIC; rec[1] = beam; rec[2] = max_frames;
    rec[3] = 1; rec[4] = 1; rec[5] = 0;
    re[0] = 0;                                       // node: the root
    re[E] = -1;                                      // last char
    re[2 * E] = __float_as_int(0.f);                 // pb
    re[3 * E] = __float_as_int(-INFINITY);           // pnb
    re[4 * E] = -1;                                  // parent
    re[5 * E] = __float_as_int(-INFINITY);           // best char log-prob
    re[6 * E] = 0;                                   // length
    re[7 * E] = 0;                                   // dictionary state: the start
    re[8 * E] = __float_as_int(0.f);                 // cached word score
    // the root's history ("<s>" throughout) is the LM's: the feed kernel supplies it on load
    const int64_t o = (int64_t)n * node_cap;
    node_parent[o] = -1; node_ch[o] = -1; node_ts[o] = -1; node_lpc[o] = -INFINITY;
    node_cnt[o] = 1; node_fc[o] = -1; node_ns[o] = -1; node_km[o] = 0ull;
  }
}

// ---------------------------------------------------------------------------
// Batched CER / WER edit distances (data/utils.py:47-57 get_cer_wer with
// decoder.py Decoder.wer / .cer): for each utterance, a = decoded ids (row n of a
// [N][a_stride] array, a_lens[n] valid), b = reference ids (flat, b_offsets/b_lens).
//   cer = Levenshtein(a without spaces, b without spaces)
//   wer = Levenshtein(words(a), words(b)), words = maximal runs of non-space ids
// out[n] = {wer, cer, max(#words(b), 1), max(#non-space(b), 1)} (ints).  Words are
// mapped to exact ids (equal length and equal ids) before the DP.  One 64-lane
// workgroup per utterance; DP rows use D[i][j] = j + prefix-min_k<=j (E[k] - k) with
// E[k] = min(D[i-1][k] + 1, D[i-1][k-1] + (x != y)), a wave scan per 64 columns.
constexpr int ED_MAXC = 2048;   // ids per sequence
constexpr int ED_MAXW = 1024;   // words per sequence

// inclusive prefix minimum over the wave in VALU only: Hillis-Steele row shifts 1, 2, 4, 8
// (lanes without a source keep their value -- min is idempotent), then row_bcast:15 / :31 carry
// the rows' minima forward.  A __shfl_up chain (six ds_bpermute round trips) made the DP row
// loop latency-bound (139 us per batch in the step)
template <int CTRL, int RMASK, int BMASK>
__device__ __forceinline__ int dpp_min_i(int v) {
  return min(v, __builtin_amdgcn_update_dpp(v, v, CTRL, RMASK, BMASK, false));
}
__device__ __forceinline__ int wave_incl_min(int v) {
  v = dpp_min_i<0x111, 0xf, 0xf>(v);   // row_shr:1
  v = dpp_min_i<0x112, 0xf, 0xf>(v);   // row_shr:2
  v = dpp_min_i<0x114, 0xf, 0xf>(v);   // row_shr:4
  v = dpp_min_i<0x118, 0xf, 0xf>(v);   // row_shr:8
  v = dpp_min_i<0x142, 0xa, 0xf>(v);   // row_bcast:15 into rows 1, 3
  v = dpp_min_i<0x143, 0xc, 0xf>(v);   // row_bcast:31 into rows 2, 3
  return v;
}

__device__ __forceinline__ int wave_excl_count(bool p, int& total) {
  const unsigned long long m = __ballot(p);
  total = __popcll(m);
  return __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0));
}

// Levenshtein distance of x[0..m) and y[0..n) (all lanes participate)
__device__ int ed_levenshtein(const int* x, int m, const int* y, int n, int* r0, int* r1) {
  const int lane = threadIdx.x;
  for (int j = lane; j <= n; j += 64) r0[j] = j;
  __syncthreads();
  int* prev = r0;
  int* cur = r1;
  for (int i = 1; i <= m; ++i) {
    const int xi = x[i - 1];
    int carry = 0x3fffffff;
    for (int j0 = 0; j0 <= n; j0 += 64) {
      const int j = j0 + lane;
      int e = 0x3fffffff;
      if (j <= n) e = j == 0 ? i : min(prev[j] + 1, prev[j - 1] + (xi != y[j - 1] ? 1 : 0));
      int v = wave_incl_min(j <= n ? e - j : 0x3fffffff);
      v = min(v, carry);
      if (j <= n) cur[j] = v + j;
      carry = __builtin_amdgcn_readlane(v, 63);
    }
    __syncthreads();
    int* tmp = prev;
    prev = cur;
    cur = tmp;
  }
  return prev[n];
}

// the same DP with the row in registers for n < 64 NC: lane l holds columns l + 64 c, D[i-1][j-1]
// comes from the next-lower lane by DPP wave_shr:1 (lane 0: column 64 c - 1 by v_readlane), so
// a row has no LDS round trip and no barrier; identical integer results
template <int NC>
__device__ int ed_levenshtein_reg(const int* x, int m, const int* y, int n) {
  const int lane = threadIdx.x;
  constexpr int BIG = 0x3fffffff;
  int prev[NC], yv[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = lane + 64 * c;
    prev[c] = j;
    yv[c] = (j >= 1 && j <= n) ? y[j - 1] : -1;
  }
  for (int i = 1; i <= m; ++i) {
    const int xi = x[i - 1];
    int carry = BIG;
    int cur[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = lane + 64 * c;
      const int lo = c == 0 ? BIG : __builtin_amdgcn_readlane(prev[c > 0 ? c - 1 : 0], 63);
      const int pj1 = __builtin_amdgcn_update_dpp(lo, prev[c], 0x138, 0xf, 0xf, false);  // wave_shr:1
      int e = BIG;
      if (j <= n) e = j == 0 ? i : min(prev[c] + 1, pj1 + (xi != yv[c] ? 1 : 0));
      int v = wave_incl_min(j <= n ? e - j : BIG);
      v = min(v, carry);
      cur[c] = v + j;
      carry = __builtin_amdgcn_readlane(v, 63);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) prev[c] = cur[c];
  }
  int r = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c == (n >> 6)) r = __builtin_amdgcn_readlane(prev[c], n & 63);
  return r;
}

__device__ __forceinline__ int ed_distance(const int* x, int m, const int* y, int n, int* r0, int* r1) {
  if (n < 64) return ed_levenshtein_reg<1>(x, m, y, n);
  if (n < 128) return ed_levenshtein_reg<2>(x, m, y, n);
  if (n < 192) return ed_levenshtein_reg<3>(x, m, y, n);
  if (n < 256) return ed_levenshtein_reg<4>(x, m, y, n);
  return ed_levenshtein(x, m, y, n, r0, r1);
}

// compact non-space ids and word starts of one sequence into LDS
__device__ void ed_tokens(const int* __restrict__ src, int len, int space, int* chars, int& nch,
                          int* wstart, int* wlen, int& nw) {
  const int lane = threadIdx.x;
  int cbase = 0, wbase = 0;
  for (int p0 = 0; p0 < len; p0 += 64) {
    const int p = p0 + lane;
    const int c = p < len ? src[p] : space;
    const int prevc = (p > 0 && p - 1 < len) ? src[p - 1] : space;
    const bool isc = p < len && c != space;
    const bool isw = isc && prevc == space;
    int tc, tw;
    const int rc = wave_excl_count(isc, tc);
    const int rw = wave_excl_count(isw, tw);
    if (isc && cbase + rc < ED_MAXC) chars[cbase + rc] = c;
    if (isw && wbase + rw < ED_MAXW) {
      int l = 0;
      while (p + l < len && src[p + l] != space) ++l;
      wstart[wbase + rw] = p;
      wlen[wbase + rw] = l;
    }
    cbase += tc;
    wbase += tw;
  }
  nch = cbase;
  nw = wbase;
}

__global__ __launch_bounds__(64) void edit_distance_kernel(
    const int* __restrict__ a, int64_t a_stride, const int* __restrict__ a_lens,
    const int* __restrict__ b, const int* __restrict__ b_offsets, const int* __restrict__ b_lens,
    int space, int* __restrict__ out, int* __restrict__ err) {
  __shared__ int ca[ED_MAXC], cb[ED_MAXC];
  __shared__ int r0[ED_MAXC + 1], r1[ED_MAXC + 1];
  __shared__ int wsa[ED_MAXW], wla[ED_MAXW], wsb[ED_MAXW], wlb[ED_MAXW];
  __shared__ int wida[ED_MAXW], widb[ED_MAXW];
  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  const int* pa = a + (int64_t)n * a_stride;
  const int* pb = b + b_offsets[n];
  const int la = a_lens[n], lb = b_lens[n];
  int nca, ncb, nwa, nwb;
  ed_tokens(pa, la, space, ca, nca, wsa, wla, nwa);
  ed_tokens(pb, lb, space, cb, ncb, wsb, wlb, nwb);
  __syncthreads();
  if (nca > ED_MAXC || ncb > ED_MAXC || nwa > ED_MAXW || nwb > ED_MAXW) {
    if (lane == 0) {
      atomicOr(err, 1);
      out[4 * n + 0] = out[4 * n + 1] = -1;
      out[4 * n + 2] = max(nwb, 1);
      out[4 * n + 3] = max(ncb, 1);
    }
    return;
  }
  // exact word ids: the index (over a's words then b's) of the first equal word
  for (int w = lane; w < nwa + nwb; w += 64) {
    const bool in_a = w < nwa;
    const int s0 = in_a ? wsa[w] : wsb[w - nwa];
    const int l0 = in_a ? wla[w] : wlb[w - nwa];
    const int* q0 = in_a ? pa + s0 : pb + s0;
    int id = w;
    for (int v = 0; v < w && id == w; ++v) {
      const bool va = v < nwa;
      const int l1 = va ? wla[v] : wlb[v - nwa];
      if (l1 != l0) continue;
      const int* q1 = va ? pa + wsa[v] : pb + wsb[v - nwa];
      bool eq = true;
      for (int k = 0; k < l0 && eq; ++k) eq = q0[k] == q1[k];
      if (eq) id = v;
    }
    if (in_a) wida[w] = id; else widb[w - nwa] = id;
  }
  __syncthreads();
  const int wer = ed_distance(wida, nwa, widb, nwb, r0, r1);
  __syncthreads();
  const int cer = ed_distance(ca, nca, cb, ncb, r0, r1);
  if (lane == 0) {
    out[4 * n + 0] = wer;
    out[4 * n + 1] = cer;
    out[4 * n + 2] = max(nwb, 1);
    out[4 * n + 3] = max(ncb, 1);
  }
}

}  // namespace ds2

using namespace ds2;

extern "C" {

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t ds2_ctc_workspace_size(int t_max, int n, int max_label_len) {
  const size_t s_max = 2 * (size_t)max_label_len + 1;
  const size_t ml = max_label_len > 0 ? max_label_len : 1;
  return al256((size_t)n * t_max * 64 * sizeof(float)) +
         2 * al256((size_t)n * t_max * s_max * sizeof(float)) + al256((size_t)n * sizeof(double)) +
         al256(2 * (size_t)n * t_max * sizeof(double)) +
         al256((size_t)n * sizeof(int)) + al256((size_t)n * 65 * sizeof(int)) +
         al256((size_t)n * ml * sizeof(int)) + 256;
}

ds2_status_t ds2_ctc_loss(const float* acts, int t_max, int n, int c, const int* labels,
                          const int* label_lens, const int* act_lens, int max_label_len,
                          int blank, int zero_infinity, float* costs, float* grads, void* ws,
                          size_t ws_bytes, ds2_stream_t stream) {
  if (t_max < 0 || n < 0 || c < 1 || c > 64 || blank < 0 || blank >= c) return DS2_INVALID_VALUE;
  if (max_label_len < 0 || max_label_len > kMaxLabel) return DS2_UNSUPPORTED_SHAPE;
  if (n == 0) return DS2_OK;
  if (ws == nullptr || ws_bytes < ds2_ctc_workspace_size(t_max, n, max_label_len))
    return DS2_WORKSPACE_TOO_SMALL;
  hipStream_t st = as_stream(stream);
  const int s_max = 2 * max_label_len + 1;
  const int ml = max_label_len > 0 ? max_label_len : 1;
  char* p = static_cast<char*>(ws);
  float* lp = reinterpret_cast<float*>(p); p += al256((size_t)n * t_max * 64 * sizeof(float));
  float* alpha = reinterpret_cast<float*>(p); p += al256((size_t)n * t_max * s_max * sizeof(float));
  float* beta = reinterpret_cast<float*>(p); p += al256((size_t)n * t_max * s_max * sizeof(float));
  double* nll = reinterpret_cast<double*>(p); p += al256((size_t)n * sizeof(double));
  double* shift = reinterpret_cast<double*>(p); p += al256(2 * (size_t)n * t_max * sizeof(double));
  int* offs = reinterpret_cast<int*>(p); p += al256((size_t)n * sizeof(int));
  int* cls_start = reinterpret_cast<int*>(p); p += al256((size_t)n * 65 * sizeof(int));
  int* cls_pos = reinterpret_cast<int*>(p);
  const int rows = t_max * n;
  if (rows > 0)
    hipLaunchKernelGGL(ctc_logsoftmax_kernel<false>, dim3(cdiv(rows, 4)), dim3(256), 0, st, acts, t_max,
                       n, c, lp);
  hipLaunchKernelGGL(ctc_prep_kernel, dim3(n), dim3(64), 0, st, labels, label_lens, n, c,
                     ml, offs, cls_start, cls_pos);
  hipLaunchKernelGGL(ctc_scan_kernel, dim3(n, 2), dim3(kScanThreads), 0, st, lp, t_max, c, labels,
                     label_lens, act_lens, offs, blank, s_max, alpha, beta, shift, nll);
  hipLaunchKernelGGL(ctc_grad_kernel, dim3(cdiv(rows > 0 ? rows : 1, 4)), dim3(256), 0, st, t_max,
                     n, c, blank, zero_infinity, act_lens, label_lens, lp, alpha, beta, shift, nll,
                     cls_start, cls_pos, s_max, ml, costs, grads);
  return launch_status("ds2_ctc_loss");
}

// log-softmax [n][t_max][64], back-pointer bytes [n][t_max][align4(2 L + 1)], then the prep
// kernel's outputs (label offsets and its class lists, which the alignment does not read)
static inline size_t align_bp_stride(int max_label_len) {
  return ((size_t)2 * max_label_len + 1 + 3) & ~(size_t)3;
}

size_t ds2_ctc_align_workspace_size(int t_max, int n, int max_label_len) {
  const size_t ml = max_label_len > 0 ? max_label_len : 1;
  return al256((size_t)n * t_max * 64 * sizeof(float)) +
         al256((size_t)n * t_max * align_bp_stride(max_label_len)) +
         al256((size_t)n * sizeof(int)) + al256((size_t)n * 65 * sizeof(int)) +
         al256((size_t)n * ml * sizeof(int)) + 256;
}

ds2_status_t ds2_ctc_align(const float* acts, int t_max, int n, int c, const int* labels,
                           const int* label_lens, const int* act_lens, int max_label_len,
                           int blank, int* states, int* spans, float* scores, void* ws,
                           size_t ws_bytes, ds2_stream_t stream) {
  if (t_max < 0 || n < 0 || c < 1 || c > 64 || blank < 0 || blank >= c) return DS2_INVALID_VALUE;
  if (max_label_len < 0 || max_label_len > kMaxLabel) return DS2_UNSUPPORTED_SHAPE;
  if (n == 0) return DS2_OK;
  if (ws == nullptr || ws_bytes < ds2_ctc_align_workspace_size(t_max, n, max_label_len))
    return DS2_WORKSPACE_TOO_SMALL;
  hipStream_t st = as_stream(stream);
  const int ml = max_label_len > 0 ? max_label_len : 1;
  const int bp_stride = static_cast<int>(align_bp_stride(max_label_len));
  char* p = static_cast<char*>(ws);
  float* lp = reinterpret_cast<float*>(p); p += al256((size_t)n * t_max * 64 * sizeof(float));
  auto* bp = reinterpret_cast<unsigned char*>(p); p += al256((size_t)n * t_max * bp_stride);
  int* offs = reinterpret_cast<int*>(p); p += al256((size_t)n * sizeof(int));
  int* cls_start = reinterpret_cast<int*>(p); p += al256((size_t)n * 65 * sizeof(int));
  int* cls_pos = reinterpret_cast<int*>(p);
  const int rows = t_max * n;
  if (rows > 0)
    hipLaunchKernelGGL(ctc_logsoftmax_kernel<true>, dim3(cdiv(rows, 4)), dim3(256), 0, st, acts, t_max,
                       n, c, lp);
  hipLaunchKernelGGL(ctc_prep_kernel, dim3(n), dim3(64), 0, st, labels, label_lens, n, c,
                     ml, offs, cls_start, cls_pos);
  hipLaunchKernelGGL(ctc_align_kernel, dim3(n), dim3(kScanThreads), 0, st, lp, t_max, c, labels,
                     label_lens, act_lens, offs, blank, max_label_len, bp_stride, bp, states,
                     spans, scores);
  return launch_status("ds2_ctc_align");
}

ds2_status_t ds2_greedy_decode(const float* probs, int n, int t_max, int c, int64_t stride_n,
                               int64_t stride_t, const int* sizes, int blank, int* out_ids,
                               int* out_offsets, int* out_counts, int* argmax_out,
                               ds2_stream_t stream) {
  if (n < 0 || t_max < 0 || c < 1 || blank < 0 || blank >= c) return DS2_INVALID_VALUE;
  if (n == 0) return DS2_OK;
  if (out_counts == nullptr) return DS2_INVALID_VALUE;
  if (t_max > 0 && (probs == nullptr || out_ids == nullptr || out_offsets == nullptr))
    return DS2_INVALID_VALUE;
  hipLaunchKernelGGL(greedy_kernel, dim3(cdiv(n, 4)), dim3(256), 0, as_stream(stream), probs, n,
                     t_max, c, stride_n, stride_t, sizes, blank, out_ids, out_offsets, out_counts,
                     argmax_out);
  return launch_status("ds2_greedy_decode");
}

// per node: parent, char, timestep, best char log-prob, cnt, first child, next sibling
// (4 bytes each) and the alive-children char mask (8 bytes)
size_t ds2_ctc_beam_workspace_size(int n, int t_max, int beam) {
  const size_t cap = (size_t)t_max * (beam > 0 ? beam : 1) + 1;
  return 7 * al256((size_t)n * cap * 4) + al256((size_t)n * cap * 8) + 256;
}

// the trie arena of n utterances of up to t_max frames inside a workspace of that size
struct BeamArena {
  int *par, *chr, *tst;
  float* lpc;
  int *cnt, *fc, *ns;
  unsigned long long* km;
  int64_t cap;   // nodes per utterance
};

static BeamArena beam_arena(void* ws, int n, int t_max, int beam_width) {
  BeamArena a;
  a.cap = (int64_t)t_max * beam_width + 1;
  char* w = static_cast<char*>(ws);
  const size_t plane = al256((size_t)n * a.cap * 4);
  a.par = reinterpret_cast<int*>(w);
  a.chr = reinterpret_cast<int*>(w + plane);
  a.tst = reinterpret_cast<int*>(w + 2 * plane);
  a.lpc = reinterpret_cast<float*>(w + 3 * plane);
  a.cnt = reinterpret_cast<int*>(w + 4 * plane);
  a.fc = reinterpret_cast<int*>(w + 5 * plane);
  a.ns = reinterpret_cast<int*>(w + 6 * plane);
  a.km = reinterpret_cast<unsigned long long*>(w + 7 * plane);
  return a;
}

static ds2_status_t beam_decode(const float* probs, int n, int t_max, int c, int64_t stride_n,
                                int64_t stride_t, const int* sizes, int blank, int beam_width,
                                int cutoff_top_n, double cutoff_prob, int top_paths,
                                int* out_ids, int* out_offsets, int* out_lens,
                                float* out_scores, void* ws, size_t ws_bytes,
                                const BeamLm* lm, ds2_stream_t stream, const char* what) {
  if (n < 0 || t_max < 0 || c < 1 || blank < 0 || blank >= c || beam_width < 1 ||
      top_paths < 1 || top_paths > beam_width || cutoff_top_n < 1)
    return DS2_INVALID_VALUE;
  const bool small = c <= BEAM_SMALL_C && beam_width <= BEAM_SMALL;
  const bool large = !small && c <= BEAM_LARGE_C && beam_width <= BEAM_LARGE;
  if (!small && !large && (c > BEAM_WIDE_C || beam_width > BEAM_WIDE))
    return DS2_UNSUPPORTED_SHAPE;
  if (n == 0) return DS2_OK;
  if (ws == nullptr || ws_bytes < ds2_ctc_beam_workspace_size(n, t_max, beam_width))
    return DS2_WORKSPACE_TOO_SMALL;
  const BeamArena a = beam_arena(ws, n, t_max, beam_width);
  BeamLm L{};
  if (lm != nullptr) L = *lm;
  L.stamps = g_beam_stamps;
  auto kern = lm != nullptr
                  ? (small   ? ctc_beam_kernel<BEAM_SMALL, BEAM_SMALL_C, true>
                     : large ? ctc_beam_kernel<BEAM_LARGE, BEAM_LARGE_C, true>
                             : ctc_beam_kernel<BEAM_WIDE, BEAM_WIDE_C, true>)
                  : (small   ? ctc_beam_kernel<BEAM_SMALL, BEAM_SMALL_C, false>
                     : large ? ctc_beam_kernel<BEAM_LARGE, BEAM_LARGE_C, false>
                             : ctc_beam_kernel<BEAM_WIDE, BEAM_WIDE_C, false>);
  hipLaunchKernelGGL(kern, dim3(n), dim3(64), 0, as_stream(stream), probs, t_max, c,
                     stride_n, stride_t, sizes, blank, beam_width, cutoff_top_n, cutoff_prob,
                     top_paths, a.par, a.chr, a.tst, a.lpc, a.cnt, a.fc, a.ns, a.km, a.cap, out_ids,
                     out_offsets, out_lens, out_scores, L, BeamStream{});
  return launch_status(what);
}

// ---- the search over a stream: [n records][trie arena for max_frames frames]
static inline size_t beam_stream_rec_words(int beam_width) {
  return BEAM_STREAM_HDR + (size_t)BEAM_STREAM_PER_ENTRY * beam_stream_entries(beam_width);
}

static inline bool beam_stream_dims_ok(int n, int max_frames, int beam_width) {
  return n >= 1 && max_frames >= 1 && beam_width >= 1 && beam_width <= BEAM_WIDE &&
         (int64_t)max_frames * beam_width + 1 <= INT32_MAX;   // node indices are ints
}

size_t ds2_ctc_beam_stream_state_size(int n, int max_frames, int beam_width) {
  if (!beam_stream_dims_ok(n, max_frames, beam_width)) return 0;
  return al256((size_t)n * beam_stream_rec_words(beam_width) * 4) +
         ds2_ctc_beam_workspace_size(n, max_frames, beam_width);
}

ds2_status_t ds2_ctc_beam_stream_init(void* state, size_t state_bytes, int n, int max_frames,
                                      int beam_width, ds2_stream_t stream) {
  if (!beam_stream_dims_ok(n, max_frames, beam_width) || state == nullptr ||
      (reinterpret_cast<uintptr_t>(state) & 255) != 0 ||
      state_bytes < ds2_ctc_beam_stream_state_size(n, max_frames, beam_width))
    return DS2_INVALID_VALUE;
  const size_t rw = beam_stream_rec_words(beam_width);
  const BeamArena a = beam_arena(static_cast<char*>(state) + al256((size_t)n * rw * 4), n,
                                 max_frames, beam_width);
  hipLaunchKernelGGL(ctc_beam_stream_init_kernel, dim3(n), dim3(64), 0, as_stream(stream),
                     static_cast<int*>(state), (int64_t)rw, beam_width, max_frames, a.par, a.chr,
                     a.tst, a.lpc, a.cnt, a.fc, a.ns, a.km, a.cap);
  return launch_status("ds2_ctc_beam_stream_init");
}

static ds2_status_t beam_stream_feed(const float* probs, int n, int t_chunk, int c,
                                     int64_t stride_n, int64_t stride_t, const int* sizes,
                                     int blank, int beam_width, int cutoff_top_n,
                                     double cutoff_prob, int top_paths, int max_frames,
                                     int t_done, int out_cap, int* out_ids, int* out_offsets,
                                     int* out_lens, float* out_scores, int* out_frames,
                                     void* state, size_t state_bytes, const BeamLm* lm,
                                     ds2_stream_t stream, const char* what) {
  if (n < 0 || t_chunk < 0 || c < 1 || blank < 0 || blank >= c || beam_width < 1 ||
      top_paths < 1 || top_paths > beam_width || cutoff_top_n < 1 || max_frames < 1 ||
      t_done < 0)
    return DS2_INVALID_VALUE;
  const bool small = c <= BEAM_SMALL_C && beam_width <= BEAM_SMALL;
  const bool large = !small && c <= BEAM_LARGE_C && beam_width <= BEAM_LARGE;
  if (!small && !large && (c > BEAM_WIDE_C || beam_width > BEAM_WIDE))
    return DS2_UNSUPPORTED_SHAPE;
  const int n_out = (out_ids != nullptr) + (out_offsets != nullptr) + (out_lens != nullptr) +
                    (out_scores != nullptr);
  if (n_out != 0 && n_out != 4) return DS2_INVALID_VALUE;
  const bool readout = n_out == 4;
  if ((int64_t)t_done + t_chunk > max_frames) return DS2_INVALID_VALUE;
  if (readout && out_cap < t_done + t_chunk) return DS2_INVALID_VALUE;
  if (n == 0 || (t_chunk == 0 && !readout)) return DS2_OK;
  if (!beam_stream_dims_ok(n, max_frames, beam_width) || state == nullptr ||
      (reinterpret_cast<uintptr_t>(state) & 255) != 0 ||
      state_bytes < ds2_ctc_beam_stream_state_size(n, max_frames, beam_width))
    return DS2_INVALID_VALUE;
  if (t_chunk > 0 && probs == nullptr) return DS2_INVALID_VALUE;
  BeamStream S;
  S.rec = static_cast<int*>(state);
  S.rec_words = (int64_t)beam_stream_rec_words(beam_width);
  S.out_frames = out_frames;
  S.max_frames = max_frames;
  S.out_cap = out_cap;
  const BeamArena a = beam_arena(static_cast<char*>(state) + al256((size_t)n * S.rec_words * 4),
                                 n, max_frames, beam_width);
  BeamLm L{};
  if (lm != nullptr) L = *lm;
  L.stamps = nullptr;
  auto kern = lm != nullptr
                  ? (small   ? ctc_beam_kernel<BEAM_SMALL, BEAM_SMALL_C, true, true>
                     : large ? ctc_beam_kernel<BEAM_LARGE, BEAM_LARGE_C, true, true>
                             : ctc_beam_kernel<BEAM_WIDE, BEAM_WIDE_C, true, true>)
                  : (small   ? ctc_beam_kernel<BEAM_SMALL, BEAM_SMALL_C, false, true>
                     : large ? ctc_beam_kernel<BEAM_LARGE, BEAM_LARGE_C, false, true>
                             : ctc_beam_kernel<BEAM_WIDE, BEAM_WIDE_C, false, true>);
  hipLaunchKernelGGL(kern, dim3(n), dim3(64), 0, as_stream(stream), probs, t_chunk, c,
                     stride_n, stride_t, sizes, blank, beam_width, cutoff_top_n, cutoff_prob,
                     top_paths, a.par, a.chr, a.tst, a.lpc, a.cnt, a.fc, a.ns, a.km, a.cap, out_ids,
                     out_offsets, out_lens, out_scores, L, S);
  return launch_status(what);
}

ds2_status_t ds2_ctc_beam_stream_feed(const float* probs, int n, int t_chunk, int c,
                                      int64_t stride_n, int64_t stride_t, const int* sizes,
                                      int blank, int beam_width, int cutoff_top_n,
                                      double cutoff_prob, int top_paths, int max_frames,
                                      int t_done, int out_cap, int* out_ids, int* out_offsets,
                                      int* out_lens, float* out_scores, int* out_frames,
                                      void* state, size_t state_bytes, ds2_stream_t stream) {
  return beam_stream_feed(probs, n, t_chunk, c, stride_n, stride_t, sizes, blank, beam_width,
                          cutoff_top_n, cutoff_prob, top_paths, max_frames, t_done, out_cap,
                          out_ids, out_offsets, out_lens, out_scores, out_frames, state,
                          state_bytes, nullptr, stream, "ds2_ctc_beam_stream_feed");
}

ds2_status_t ds2_ctc_beam_decode(const float* probs, int n, int t_max, int c, int64_t stride_n,
                                 int64_t stride_t, const int* sizes, int blank, int beam_width,
                                 int cutoff_top_n, double cutoff_prob, int top_paths,
                                 int* out_ids, int* out_offsets, int* out_lens,
                                 float* out_scores, void* ws, size_t ws_bytes,
                                 ds2_stream_t stream) {
  return beam_decode(probs, n, t_max, c, stride_n, stride_t, sizes, blank, beam_width,
                     cutoff_top_n, cutoff_prob, top_paths, out_ids, out_offsets, out_lens,
                     out_scores, ws, ws_bytes, nullptr, stream, "ds2_ctc_beam_decode");
}

// the LM arguments of the _lm entry points, checked and gathered; false = DS2_INVALID_VALUE
static bool beam_lm_args(int c, int blank, int space_id, int lm_order, int start_id, int lm_vocab,
                         double alpha, double beta, const int* dict_next, const void* dict_mask,
                         const int* dict_word, int dict_states, int dict_cols,
                         const int* lm_table, int64_t lm_slots, BeamLm& L) {
  if (space_id < 0 || space_id >= c || space_id == blank || lm_order < 1 ||
      lm_order > LM_MAX_ORDER || start_id < 0 || start_id >= lm_vocab || dict_states < 2 ||
      dict_cols != c || dict_next == nullptr ||
      dict_mask == nullptr || dict_word == nullptr || lm_table == nullptr || lm_slots < 1 ||
      (lm_slots & (lm_slots - 1)) != 0 || lm_slots > (int64_t(1) << 31) || c > 64)
    return false;
  L.dnext = dict_next;
  L.dmask = static_cast<const unsigned long long*>(dict_mask);
  L.dword = dict_word;
  L.tab = reinterpret_cast<const int4*>(lm_table);
  L.tmask = static_cast<unsigned>(lm_slots - 1);
  L.fstate = dict_states - 1;
  L.nstates = dict_states;
  L.order = lm_order;
  L.start = start_id;
  L.space = space_id;
  L.alpha = alpha;
  L.beta = beta;
  L.stamps = nullptr;
  return true;
}

ds2_status_t ds2_ctc_beam_decode_lm(const float* probs, int n, int t_max, int c, int64_t stride_n,
                                    int64_t stride_t, const int* sizes, int blank, int beam_width,
                                    int cutoff_top_n, double cutoff_prob, int top_paths,
                                    int space_id, int lm_order, int start_id, int lm_vocab,
                                    double alpha, double beta, const int* dict_next,
                                    const void* dict_mask, const int* dict_word, int dict_states,
                                    int dict_cols, const int* lm_table, int64_t lm_slots,
                                    int* out_ids, int* out_offsets, int* out_lens,
                                    float* out_scores, void* ws, size_t ws_bytes,
                                    ds2_stream_t stream) {
  BeamLm L;
  if (!beam_lm_args(c, blank, space_id, lm_order, start_id, lm_vocab, alpha, beta, dict_next,
                    dict_mask, dict_word, dict_states, dict_cols, lm_table, lm_slots, L))
    return DS2_INVALID_VALUE;
  return beam_decode(probs, n, t_max, c, stride_n, stride_t, sizes, blank, beam_width,
                     cutoff_top_n, cutoff_prob, top_paths, out_ids, out_offsets, out_lens,
                     out_scores, ws, ws_bytes, &L, stream, "ds2_ctc_beam_decode_lm");
}

ds2_status_t ds2_ctc_beam_stream_feed_lm(const float* probs, int n, int t_chunk, int c,
                                         int64_t stride_n, int64_t stride_t, const int* sizes,
                                         int blank, int beam_width, int cutoff_top_n,
                                         double cutoff_prob, int top_paths, int space_id,
                                         int lm_order, int start_id, int lm_vocab, double alpha,
                                         double beta, const int* dict_next, const void* dict_mask,
                                         const int* dict_word, int dict_states, int dict_cols,
                                         const int* lm_table, int64_t lm_slots, int max_frames,
                                         int t_done, int out_cap, int* out_ids, int* out_offsets,
                                         int* out_lens, float* out_scores, int* out_frames,
                                         void* state, size_t state_bytes, ds2_stream_t stream) {
  BeamLm L;
  if (!beam_lm_args(c, blank, space_id, lm_order, start_id, lm_vocab, alpha, beta, dict_next,
                    dict_mask, dict_word, dict_states, dict_cols, lm_table, lm_slots, L))
    return DS2_INVALID_VALUE;
  return beam_stream_feed(probs, n, t_chunk, c, stride_n, stride_t, sizes, blank, beam_width,
                          cutoff_top_n, cutoff_prob, top_paths, max_frames, t_done, out_cap,
                          out_ids, out_offsets, out_lens, out_scores, out_frames, state,
                          state_bytes, &L, stream, "ds2_ctc_beam_stream_feed_lm");
}

ds2_status_t ds2_test_beam_stamps(unsigned long long* buf) {
  g_beam_stamps = buf;   // [BEAM_NSTAMP_T][BEAM_NSTAMP_P] device buffer, or null
  return DS2_OK;
}

ds2_status_t ds2_edit_distance(const int* a_ids, int64_t a_stride, const int* a_lens,
                               const int* b_ids, const int* b_offsets, const int* b_lens, int n,
                               int space_id, int* out, int* err, ds2_stream_t stream) {
  if (n < 0 || a_stride < 0) return DS2_INVALID_VALUE;
  if (n == 0) return DS2_OK;
  if (a_ids == nullptr || a_lens == nullptr || b_ids == nullptr || b_offsets == nullptr ||
      b_lens == nullptr || out == nullptr || err == nullptr)
    return DS2_INVALID_VALUE;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(n), dim3(64), 0, as_stream(stream), a_ids,
                     a_stride, a_lens, b_ids, b_offsets, b_lens, space_id, out, err);
  return launch_status("ds2_edit_distance");
}

}  // extern "C"
