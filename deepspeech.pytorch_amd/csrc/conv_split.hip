// Conv2d on the bf16 / fp16 matrix cores at fp32 accuracy: the split-operand kernel families
// (bf16x6: three bf16 terms per operand, six products; fp16x3: two scaled fp16 terms, three
// products) and the launchers of their rungs (launch_conv_split*, at the end), which conv.hip's
// entry points call with the plan conv_host.h made.  In file order:
//   * the MFMA groups on its fragments (cx_mma*: split_mma.h's), the fp16x3 scale kernels
//     (conv_h3_wexp_kernel, conv_h3_samax_kernel, conv_h3_chamax_kernel);
//   * forward and 8-row-fragment dgrad, one output row per workgroup (conv_x6_wimg_kernel,
//     conv_x6_kernel), and conv2's two-row fp16x3 forward (conv_h3_fwd2r_kernel);
//   * the weight gradients for 11 kernel columns: per-row re-staging (conv_x6_wgrad_kernel),
//     the sliding window (conv_x6_wgrad_sw_kernel) and their reduction (wgrad_reduce_x6_kernel);
//   * the 4 x 2-fragment dgrad (conv_x6q_wimg_kernel, conv_x6q_dgrad_kernel) and conv2's
//     two-row fp16x3 dgrad (conv_h3_dgrad2r_kernel).
#include "conv_host.h"

namespace ds2 {

// ---------------------------------------------------------------------------
// bf16x6 direct convolution, forward (width stride 1 or 2) and dgrad (width stride 1), on the
// bf16 matrix cores at
// fp32 accuracy: every fp32 operand value is split into hi / mid / lo bf16 terms and a
// product is formed from the six terms that carry fp32 weight (gemm.hip sxgemm_kernel), on
// v_mfma_f32_32x32x16_bf16: M = 32 output channels, N = 32 output columns, K = 16 taps.
//
// K order: tap rows a in runs of 8 (a-group g) x kernel columns b in pairs (p): lane half
// h of the MFMA takes b = 2p + h and a = 8g .. 8g + 7, so its 8 k values are 8 consecutive
// input ROWS of one input column -- contiguous in a column-major LDS patch (16-B aligned,
// one ds_read_b128 per plane), and 8 consecutive a of one (m, b) in the weight image.
// Taps past the kernel (a >= rows of taps, b >= kw) have zero weight.  More than 24 tap rows
// (conv1's 41) run as chunks of 16 rows, each staged like a loop channel of its own (RC
// chunks per channel); width stride 2 reads patch column 2 (output column) + b.
//   fwd  : out y[n][co][ho][wo], loop channels ci, input row ho*sh - ph + a, col wo - pw + b
//   dgrad: out dx[n][ci][hi][wi] for hi of stride class q, loop channels co, taps of the
//          class reversed (dy row (hi + ph - q)/sh - (A_q - 1) + a, col wi + pw - kw + 1 + b)
// Workgroup: one output row x 256 columns x 32 output channels; 8 waves = 4 column
// quarters (64 columns, 2 MFMA tiles) x 2 halves of the k-steps, whose partial sums meet in
// LDS once at the end.  Per loop channel the input patch (KA rows x 256 + 2 NBP - 1
// columns) is split and stored column-major (pitch P = 8 x odd bf16: conflict-free
// fragment reads) and the channel's pre-split weight image [3][32][COP] is copied in; the
// next channel's global loads fly during the MFMAs.

// The planes of either format are read as bf16x8 fragments; fp16x3's are bit-cast for the MFMA.
__device__ __forceinline__ f16x8 as_h(bf16x8 v) { return __builtin_bit_cast(f16x8, v); }

// acc += a.b over one 32 x 32 x 16 fragment pair: bf16x6 or fp16x3 in one chain
template <int NPL>
__device__ __forceinline__ f32x16 cx_mma(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 c) {
  if constexpr (NPL == 2) return mma3h(as_h(a[0]), as_h(a[1]), as_h(b[0]), as_h(b[1]), c);
  else return mma6(a, b, c);
}

// fp16x3 with the small products in their own chain (split_mma.h, the product order): the sums
// of the outputs that the conv block's BatchNorm parameter gradients take amplify their bias
__device__ __forceinline__ void cx_mma_h3s(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16& big,
                                           f32x16& small) {
  mma3h2(as_h(a[0]), as_h(a[1]), as_h(b[0]), as_h(b[1]), big, small);
}

// fp16x3 scales of an implicit-GEMM convolution: m_exp[m] = h3_exp(max |w| over the taps and
// loop channels of output row m) (fwd: m = co; dgrad: m = ci), one workgroup per m
template <bool DGRAD>
__global__ void conv_h3_wexp_kernel(const float* __restrict__ w, ConvDims g, int* __restrict__ m_exp) {
  __shared__ float red[4];
  const int m = blockIdx.x;
  const int KHW = g.kh * g.kw;
  const int L = DGRAD ? g.co : g.ci;
  float mx = 0.f;
  for (int i = threadIdx.x; i < L * KHW; i += blockDim.x) {
    const int l = i / KHW, t = i - l * KHW;
    const float v = DGRAD ? w[((int64_t)l * g.ci + m) * KHW + t] : w[((int64_t)m * g.ci + l) * KHW + t];
    mx = fmaxf(mx, fabsf(v));
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) mx = fmaxf(mx, red[i]);
    m_exp[m] = h3_exp(__float_as_uint(mx));
  }
}

// per-sample max |x| of an [n][per] tensor (float bits, unsigned atomic max; out zeroed first):
// grid (chunks, n), 256 threads, 16-B loads where the sample's base is 16-B aligned
__global__ void conv_h3_samax_kernel(const float* __restrict__ x, int64_t per,
                                     unsigned* __restrict__ out) {
  __shared__ float red[4];
  const int n = blockIdx.y;
  const float* xs = x + (int64_t)n * per;
  // chunks of a multiple of 4 elements, so that 16-B aligned samples take the float4 path
  const int64_t chunk = (((per + gridDim.x - 1) / gridDim.x) + 3) & ~(int64_t)3;
  const int64_t b = (int64_t)blockIdx.x * chunk;
  const int64_t e = b + chunk < per ? b + chunk : per;
  if (b >= e) return;   // block-uniform: past the sample's end after the rounding up
  float mx = 0.f;
  if ((reinterpret_cast<uintptr_t>(xs + b) & 15) == 0) {
    const int64_t e4 = b + ((e - b) & ~(int64_t)3);
    // unrolled: 8 loads in flight per thread (one at a time ran at ~2.5 TB/s)
#pragma unroll 8
    for (int64_t i = b + 4 * threadIdx.x; i < e4; i += 4 * blockDim.x) {
      const float4 v = *reinterpret_cast<const float4*>(xs + i);
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    for (int64_t i = e4 + threadIdx.x; i < e; i += blockDim.x) mx = fmaxf(mx, fabsf(xs[i]));
  } else {
#pragma unroll 8
    for (int64_t i = b + threadIdx.x; i < e; i += blockDim.x) mx = fmaxf(mx, fabsf(xs[i]));
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) mx = fmaxf(mx, red[i]);
    if (b < e) atomicMax(out + n, __float_as_uint(mx));
  }
}

// per-channel max |t| of an [N][C][plane] tensor (float bits, unsigned atomic max; out zeroed
// first): grid (chunks, C), 256 threads striding the channel's N x plane elements
__global__ void conv_h3_chamax_kernel(const float* __restrict__ t, int N, int C, int64_t plane,
                                      unsigned* __restrict__ out) {
  __shared__ float red[4];
  const int ch = blockIdx.y;
  const int64_t total = (int64_t)N * plane;
  const int64_t chunk = (total + gridDim.x - 1) / gridDim.x;
  const int64_t b = (int64_t)blockIdx.x * chunk;
  const int64_t e = b + chunk < total ? b + chunk : total;
  float mx = 0.f;
  // the chunk walked sample by sample: inside one sample the channel's plane is contiguous,
  // so the loop is a plain strided sweep with 8 loads in flight per thread
  for (int64_t i = b; i < e;) {
    const int64_t n = i / plane;
    const int64_t seg = (n + 1) * plane < e ? (n + 1) * plane : e;
    const float* base = t + (n * C + ch) * plane - n * plane;   // base[k]: element k
#pragma unroll 8
    for (int64_t k = i + threadIdx.x; k < seg; k += blockDim.x) mx = fmaxf(mx, fabsf(base[k]));
    i = seg;
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) mx = fmaxf(mx, red[k]);
    if (b < e && mx > 0.f) atomicMax(out + ch, __float_as_uint(mx));
  }
}

// split-weight image: [class][mb][loop channel][plane][32][COP] bf16 (NPL 3) or fp16 (NPL 2)
// NPL 2: fp16 hi / lo planes of w 2^m_exp[m] (fp16x3)
template <bool DGRAD, int NPL = 3>
__global__ void conv_x6_wimg_kernel(const float* __restrict__ w, ConvDims g, CxGeom c,
                                    unsigned short* __restrict__ img,
                                    const int* __restrict__ m_exp, int flip_odd = 0) {
  const int M = DGRAD ? g.ci : g.co;
  const int L = (DGRAD ? g.co : g.ci) * c.RC;          // (channel, tap-row chunk) pairs
  const int mbn = (M + 31) / 32;
  const int classes = DGRAD ? g.sh : 1;
  const int64_t per = (int64_t)32 * c.COP;             // one plane of one (class, mb, l)
  const int64_t total = (int64_t)classes * mbn * L * per;
  const int KHW = g.kh * g.kw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int e = static_cast<int>(r % per); r /= per;
    const int l = static_cast<int>(r % L); r /= L;
    const int mb = static_cast<int>(r % mbn); r /= mbn;
    const int q = static_cast<int>(r);
    const int mm = e / c.COP, rem = e - mm * c.COP;
    const int b = rem / c.KA, al = rem - b * c.KA;
    const int m = mb * 32 + mm;
    const int ch = l / c.RC, a = (l - ch * c.RC) * c.KA + al;
    float v = 0.f;
    if (rem < 2 * c.NBP * c.KA && m < M && b < g.kw) {
      if (!DGRAD) {
        if (a < g.kh) v = w[((int64_t)m * g.ci + ch) * KHW + a * g.kw + b];
      } else {
        const int aq = class_taps(g, q);
        if (a < aq) v = w[((int64_t)ch * g.ci + m) * KHW + (q + g.sh * (aq - 1 - a)) * g.kw + (g.kw - 1 - b)];
      }
      // k-step st = (tap-row group, column pair); the second half of the k-steps (the kk = 1
      // waves' share) is stored negated: see conv_x6_kernel's epilogue.  flip_odd 1: the odd
      // loop channels instead; 2: nothing negated (conv_h3_fwd2r_kernel)
      const int st = (al >> 3) * c.NBP + (b >> 1), nks = (c.KA / 8) * c.NBP;
      if (flip_odd == 0 ? st >= (nks + 1) / 2 : (flip_odd == 1 && (l & 1) != 0)) v = -v;
    }
    const float sc = NPL == 2 && m < M ? h3_scale(m_exp[m]) : 1.f;
    split_put<NPL>(img, ((((int64_t)q * mbn + mb) * L + l) * NPL) * per + e, per, v, sc);
  }
}

// NGA, NBP > 0: compile-time a-groups / column pairs (fully unrolled k loop for the model's
// conv2: fwd 3 x 6, dgrad 2 x 6; conv1 fwd 2 x 6); 0: read from c at run time.  PU: patch
// staging units per thread (2, or 3 for conv1's 522-column stride-2 patch).  SW: width stride
// (0: run time); RCH: tap-row chunks (c.RC) possible.  The width-stride-1 unchunked form
// (conv2) keeps its smaller LDS patch and compile-time addressing.
// DB: the input patch double-buffered (conv2 fwd): the next channel's patch is split and
// stored into the other buffer in the middle of this channel's k-steps (its loads were issued
// at the channel's start), so only the weight image copy stays between the two barriers.
// NPL 2: fp16x3 -- the patch is staged as fp16 hi / lo of x 2^e_n (e_n from the sample's
// max |x|, n_amax[n]), the image holds w 2^m_exp[m], three products per fragment pair, and the
// epilogue multiplies by 2^-(m_exp[m] + e_n) (exact) before the bias.
template <bool DGRAD, int NGA, int NBP_, int PU, int SW, bool RCH, bool DB = false, int NPL = 3>
__global__ __launch_bounds__(CX_T, 1) void conv_x6_kernel(const float* __restrict__ in,
                                                          const unsigned short* __restrict__ img,
                                                          const float* __restrict__ bias,
                                                          float* __restrict__ out, ConvDims g,
                                                          const int* __restrict__ out_lens,
                                                          CxGeom c, int gx, int gy,
                                                          const int* __restrict__ m_exp,
                                                          const unsigned* __restrict__ n_amax) {
  __shared__ __attribute__((aligned(16))) unsigned short
      ps[DB ? CX_PATCH_DB : ((SW == 1 && !RCH) ? CX_PATCH1 : CX_PATCH)];
  __shared__ __attribute__((aligned(16))) unsigned short ws[CX_WIMG];
  const int M = DGRAD ? g.ci : g.co;
  const int L = DGRAD ? g.co : g.ci;
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
  const int c0 = bx * CX_COLS;
  // output row and the first input row of its taps
  int orow, prow0, q = 0, A;
  if (!DGRAD) {
    orow = by;
    prow0 = orow * g.sh - g.ph;
    A = g.kh;
  } else {
    int t = by, hq = 0;
    for (q = 0; q < g.sh; ++q) {
      hq = ((q - g.ph) % g.sh + g.sh) % g.sh;
      const int cnt = hq < g.hi ? (g.hi - 1 - hq) / g.sh + 1 : 0;
      if (t < cnt) break;
      t -= cnt;
    }
    A = class_taps(g, q);
    orow = hq + g.sh * t;
    prow0 = (orow + g.ph - q) / g.sh - (A - 1);
  }
  const int sw = DGRAD ? 1 : (SW > 0 ? SW : g.sw);
  const int pcol0 = DGRAD ? c0 + g.pw - g.kw + 1 : c0 * sw - g.pw;
  const int RC = RCH ? c.RC : 1;
  const int LL = L * RC;                       // staged (channel, tap-row chunk) pairs
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cw = wave & 3, kk = wave >> 2;
  const int plane_in = in_h * in_w;
  const float* inn = in + (int64_t)n * L * plane_in;
  constexpr bool CG = NGA > 0 && NBP_ > 0 && SW == 1 && !RCH;   // compile-time geometry
  using CC = CxConst<(NGA > 0 ? NGA : 1), (NBP_ > 0 ? NBP_ : 1)>;
  const int cP = CG ? CC::P : c.P;
  const int cCOP = CG ? CC::COP : c.COP;
  const int cKA = CG ? CC::KA : c.KA;
  const int cPCOL = CG ? CC::PCOL : c.PCOL;
  const int PPL = cPCOL * cP;                  // bf16 per patch plane
  const int WPL = 32 * cCOP;                   // bf16 per weight plane
  const int64_t wstride = (int64_t)NPL * WPL;  // one loop channel's image
  const int en = NPL == 2 ? h3_exp(n_amax[n]) : 0;
  const float nsc = h3_scale(en);
  const unsigned short* wimg = img + ((int64_t)q * mbn + mb) * L * RC * wstride;
  const int ngr = NGA > 0 ? NGA : cKA / 8;
  const int nbp = NBP_ > 0 ? NBP_ : c.NBP;
  const int units = cPCOL * ngr;
  const int wchunks = (int)(wstride / 8);

  float rp[PU][8];
  u32x4 rw[CX_WQ];
  auto load_w = [&](int l) {
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(wimg + (int64_t)l * wstride), (short)0,
        static_cast<int>(wstride * 2), 0x00020000);
#pragma unroll
    for (int r = 0; r < CX_WQ; ++r) {
      const int i = tid + CX_T * r;
      rw[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                            wr, i < wchunks ? i * 16 : 0x7ffffff0, 0, 0));
    }
  };
  auto load = [&](int l) {
    const int ch = RCH ? l / RC : l, ar0 = RCH ? (l - ch * RC) * cKA : 0;   // chunk's first tap row
    const __amdgpu_buffer_rsrc_t rs = conv_rsrc(inn + (int64_t)ch * plane_in, plane_in);
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int unit = tid + CX_T * u;
      const int j = unit / ngr, rg = unit - (unit / ngr) * ngr;
      const int ic = pcol0 + j;
      const bool cok = unit < units && ic >= 0 && ic < in_w;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int a = ar0 + 8 * rg + i, ir = prow0 + a;
        const bool ok = cok && a < A && ir >= 0 && ir < in_h;
        rp[u][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                 rs, ok ? (ir * in_w + ic) * 4 : 0x7ffffff0, 0, 0));
      }
    }
    if (!DB) load_w(l);
  };
  auto store_patch = [&](unsigned short* dst) {
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int unit = tid + CX_T * u;
      if (unit < units) {
        const int j = unit / ngr, rg = unit - (unit / ngr) * ngr;
        split_store8<NPL>(dst, PPL, j * cP + 8 * rg, rp[u], nsc);
      }
    }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int r = 0; r < CX_WQ; ++r) {
      const int i = tid + CX_T * r;
      if (i < wchunks) *reinterpret_cast<u32x4*>(ws + 8 * i) = rw[r];
    }
  };
  auto store = [&]() {
    store_patch(ps);
    store_w();
  };

  f32x16 acc[2], acs[2];   // acs: fp16x3's small products (cx_mma_h3s)
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = acs[j][r] = 0.f;
  const int nks = ngr * nbp;
  const int s_beg = kk == 0 ? 0 : (nks + 1) / 2;
  const int s_end = kk == 0 ? (nks + 1) / 2 : nks;
  const int fr = lane & 31, fh = lane >> 5;
  const bool active = orow < out_h && c0 + 64 * cw < out_w;

  load(0);
  if (DB) load_w(0);
  store();
  __syncthreads();
  for (int l = 0; l < LL; ++l) {
    if (l + 1 < LL) load(l + 1);
    const unsigned short* pcur = DB ? ps + (l & 1) * NPL * PPL : ps;
    unsigned short* pnext = ps + ((l + 1) & 1) * NPL * PPL;
    bool staged = false;
    if (active) {
      auto kstep = [&](int st) {
        const int ga = st / nbp, p = st - (st / nbp) * nbp;
        const int b = 2 * p + fh;
        bf16x8 af[3], bfr[2][3];
        const int aw = fr * cCOP + b * cKA + 8 * ga;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) af[pl] = *reinterpret_cast<const bf16x8*>(ws + pl * WPL + aw);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int ap = ((64 * cw + 32 * j + fr) * sw + b) * cP + 8 * ga;
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl)
            bfr[j][pl] = *reinterpret_cast<const bf16x8*>(pcur + pl * PPL + ap);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (NPL == 2) cx_mma_h3s(af, bfr[j], acc[j], acs[j]);
          else acc[j] = cx_mma<NPL>(af, bfr[j], acc[j]);
        }
      };
      if (NGA > 0 && NBP_ > 0) {
        constexpr int NK = NGA * NBP_, H0 = (NK + 1) / 2;
        constexpr int MID = H0 / 2 + 1;     // DB: stage the next patch after these k-steps
        if (kk == 0) {
#pragma unroll
          for (int st = 0; st < H0; ++st) {
            if (DB && st == MID && l + 1 < LL) {
              store_patch(pnext);
              load_w(l + 1);        // issued once rp is free: rp and rw never live together
              staged = true;
            }
            kstep(st);
            if (DB) __builtin_amdgcn_sched_barrier(0);   // bound the fragment-read hoisting
          }
        } else {
#pragma unroll
          for (int st = H0; st < NK; ++st) {
            if (DB && st == H0 + MID && l + 1 < LL) {
              store_patch(pnext);
              load_w(l + 1);
              staged = true;
            }
            kstep(st);
            if (DB) __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else {
        for (int st = s_beg; st < s_end; ++st) kstep(st);
      }
    }
    if (DB && !staged && l + 1 < LL) {
      store_patch(pnext);
      load_w(l + 1);
    }
    __syncthreads();
    if (l + 1 < LL) {
      if (DB) {
        store_w();
      } else {
        store();
      }
      __syncthreads();
    }
  }
  if constexpr (NPL == 2) {
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j] += acs[j];
  }
  // the two k halves meet in LDS (the patch area): half 1 writes, half 0 adds (fixed order).
  // Sign split: half 1 ran on the negated weight image (its chains hold -(its sum)), so the
  // MFMAs' toward -inf rounding of low addend bits (profiles/r5n_mfma_rounding.txt) drifts
  // the two halves' contributions in opposite directions and they cancel to their difference.
  float* red = reinterpret_cast<float*>(ps);
  if (kk == 1) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((cw * 2 + j) * 16 + r) * 64 + lane] = acc[j][r];
  }
  __syncthreads();
  if (kk == 1 || !active) return;
  const int len = (!DGRAD && out_lens != nullptr) ? out_lens[n] : out_w;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = c0 + 64 * cw + 32 * j + fr;
    if (col >= out_w) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      if (m < M) {
        float v = acc[j][r] - red[((cw * 2 + j) * 16 + r) * 64 + lane];   // sign split
        if (NPL == 2) v = __builtin_ldexpf(v, -(m_exp[m] + en));
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
// conv2 forward on fp16x3, two output rows per workgroup (height stride 2, width stride 1,
// <= 24 tap rows, 6 kernel-column pairs: the model's 21 x 11 conv2).  With stride 2, output
// rows r and r + 4 read input rows 8 apart -- exactly one 8-row fragment group -- so ONE
// column-major patch of 32 input rows serves both: row r's B fragments are patch row groups
// 0..2, row r + 4's are groups 1..3, and both multiply the SAME weight fragments (tap row group
// ga).  Per loop channel a workgroup then stages 32 patch rows and one weight image for two
// output rows (conv_x6_kernel: 24 rows and one image for one row), and every weight fragment
// read feeds six MFMAs instead of three.  Rows r, r + 4 with r = 8 b + j (j < 4) tile the
// output rows in pairs; a row past the output is computed and not stored.
// Waves: 8 x 32 columns, each all 18 k-steps of both rows (no k halves).  The sign split of
// conv_x6_kernel (one k half on negated weights) becomes a sign per loop channel: the weight
// image stores odd channels negated, both MFMA chains (hi.hi and the small products,
// cx_mma_h3s) restart from zero every channel and are folded into a VALU total with the
// channel's sign, so the MFMAs' floor of low addend bits drifts one way in even channels and
// the other in odd ones and cancels in the total (DESIGN.md §4 "MFMA rounding", which also
// records the two forms tried before this one).  The next channel's patch is double-buffered
// as in conv_x6_kernel.
constexpr int C2_KAP = 32;                                  // patch rows
constexpr int C2_P = cx_pitch8odd(C2_KAP);                  // 40: 8 x odd bf16
constexpr int C2_PCOL = CxConst<3, 6>::PCOL;                // 267
constexpr int C2_PPL = C2_PCOL * C2_P;                      // fp16 per patch plane
constexpr int C2_WPL = 32 * CxConst<3, 6>::COP;             // fp16 per weight plane
constexpr int C2_WQ = (2 * C2_WPL / 8 + CX_T - 1) / CX_T;   // 16-B image chunks per thread
constexpr int C2_PU = (C2_PCOL * (C2_KAP / 8) + CX_T - 1) / CX_T;   // patch units per thread

__global__ __launch_bounds__(CX_T, 1) void conv_h3_fwd2r_kernel(
    const float* __restrict__ in, const unsigned short* __restrict__ img,
    const float* __restrict__ bias, float* __restrict__ out, ConvDims g,
    const int* __restrict__ out_lens, int gx, int gy, const int* __restrict__ m_exp,
    const unsigned* __restrict__ n_amax) {
  using CC = CxConst<3, 6>;
  __shared__ __attribute__((aligned(16))) unsigned short ps[2 * 2 * C2_PPL];
  __shared__ __attribute__((aligned(16))) unsigned short ws[2 * C2_WPL];
  const int M = g.co, L = g.ci;
  const int mbn = (M + 31) / 32;
  int bx, by, bz;
  xcd_tile(gx, gy, bx, by, bz);
  const int n = bz / mbn;
  const int mb = bz - n * mbn;
  const int m0 = mb * 32;
  const int c0 = bx * CX_COLS;
  const int orow = 8 * (by >> 2) + (by & 3);          // and orow + 4
  const int prow0 = orow * 2 - g.ph;                   // the patch's first input row
  const int pcol0 = c0 - g.pw;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plane_in = g.hi * g.wi;
  const float* inn = in + (int64_t)n * L * plane_in;
  const int en = h3_exp(n_amax[n]);
  const float nsc = h3_scale(en);
  constexpr int wstride = 2 * C2_WPL;                  // one loop channel's image (fp16)
  const unsigned short* wimg = img + (int64_t)mb * L * wstride;
  constexpr int wchunks = wstride / 8;
  constexpr int units = C2_PCOL * (C2_KAP / 8);
  const int last_row = 2 * 4 + 20;                     // rows a >= 29 feed no tap of either row

  float rp[C2_PU][8];
  u32x4 rw[C2_WQ];
  auto load_w = [&](int l) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(wimg + (int64_t)l * wstride), (short)0, wstride * 2, 0x00020000);
#pragma unroll
    for (int r = 0; r < C2_WQ; ++r) {
      const int i = tid + CX_T * r;
      rw[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                            wr, i < wchunks ? i * 16 : 0x7ffffff0, 0, 0));
    }
  };
  auto load = [&](int l) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t rs = conv_rsrc(inn + (int64_t)l * plane_in, plane_in);
#pragma unroll
    for (int u = 0; u < C2_PU; ++u) {
      const int unit = tid + CX_T * u;
      const int j = unit >> 2, rg = unit & 3;
      const int ic = pcol0 + j;
      const bool cok = unit < units && ic >= 0 && ic < g.wi;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int a = 8 * rg + i, ir = prow0 + a;
        const bool ok = cok && a <= last_row && ir >= 0 && ir < g.hi;
        rp[u][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                 rs, ok ? (ir * g.wi + ic) * 4 : 0x7ffffff0, 0, 0));
      }
    }
  };
  auto store_patch = [&](unsigned short* dst) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < C2_PU; ++u) {
      const int unit = tid + CX_T * u;
      if (unit < units) split_store8<2>(dst, C2_PPL, (unit >> 2) * C2_P + 8 * (unit & 3), rp[u], nsc);
    }
  };
  auto store_w = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < C2_WQ; ++r) {
      const int i = tid + CX_T * r;
      if (i < wchunks) *reinterpret_cast<u32x4*>(ws + 8 * i) = rw[r];
    }
  };

  f32x16 acc[2], acs[2];
  f32x16 tot[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[j][r] = acs[j][r] = 0.f;
      tot[j][r] = 0.f;
    }
  const int fr = lane & 31, fh = lane >> 5;
  const bool active = c0 + 32 * wave < g.wo;

  load(0);
  load_w(0);
  store_patch(ps);
  store_w();
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    if (l + 1 < L) load(l + 1);
    const unsigned short* pcur = ps + (l & 1) * 2 * C2_PPL;
    unsigned short* pnext = ps + ((l + 1) & 1) * 2 * C2_PPL;
    bool staged = false;
    if (active) {
      constexpr int NK = 3 * 6, MID = 6;
#pragma unroll
      for (int st = 0; st < NK; ++st) {
        if (st == MID && l + 1 < L) {
          store_patch(pnext);
          load_w(l + 1);
          staged = true;
        }
        const int ga = st / 6, p = st - (st / 6) * 6;
        const int b = 2 * p + fh;
        bf16x8 af[3], b0[3], b1[3];
        const int aw = fr * CC::COP + b * CC::KA + 8 * ga;
        const int ap = (32 * wave + fr + b) * C2_P + 8 * ga;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          af[pl] = *reinterpret_cast<const bf16x8*>(ws + pl * C2_WPL + aw);
          b0[pl] = *reinterpret_cast<const bf16x8*>(pcur + pl * C2_PPL + ap);
          b1[pl] = *reinterpret_cast<const bf16x8*>(pcur + pl * C2_PPL + ap + 8);
        }
        cx_mma_h3s(af, b0, acc[0], acs[0]);
        cx_mma_h3s(af, b1, acc[1], acs[1]);
        __builtin_amdgcn_sched_barrier(0);   // bound the fragment-read hoisting
      }
    }
    if (!staged && l + 1 < L) {
      store_patch(pnext);
      load_w(l + 1);
    }
    // both chains restart every channel and are folded into a VALU sum (RNE); odd channels
    // ran on the negated weight image, so they are subtracted
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (l & 1) tot[j] -= acc[j] + acs[j];
      else tot[j] += acc[j] + acs[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = acs[j][r] = 0.f;
    }
    __syncthreads();
    if (l + 1 < L) {
      store_w();
      __syncthreads();
    }
  }
  if (!active) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    acc[j] = tot[j];
#pragma unroll
    for (int r = 0; r < 16; ++r) acs[j][r] = 0.f;
  }
  const int len = out_lens != nullptr ? out_lens[n] : g.wo;
  const int col = c0 + 32 * wave + fr;
  if (col >= g.wo) return;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int row = orow + 4 * rr;
    if (row >= g.ho) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      if (m < M) {
        float v = __builtin_ldexpf(acc[rr][r] + acs[rr][r], -(m_exp[m] + en));
        if (bias != nullptr) v += bias[m];
        if (col >= len) v = 0.f;
        out[(((int64_t)n * M + m) * g.ho + row) * g.wo + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// bf16x6 weight gradient (width stride 1, <= 32 input and output channels; instantiated for
// the model's conv2 columns: kw = 11, pw = 5) on v_mfma_f32_32x32x16_bf16 at fp32 accuracy:
//   dW[co][ci][a][b] = sum over (n, ho, wo) of dy[n][co][ho][wo] x[n][ci][ho sh - ph + a][wo - pw + b]
// For ONE tap (a, b) this is a 32 x 32 (co x ci) product over positions: M = co, N = ci,
// K = 16 consecutive output columns.  Wave w of a workgroup owns tap row a = 4 gi + w and all
// kw kernel columns (kw accumulators).  Its A fragment (dy: 8 consecutive columns of one co,
// one ds_read_b128 per plane) serves all kw taps; the B fragments of the kw taps are windows
// at offsets b + 8 - pw into 24 consecutive x columns of one ci (three aligned ds_read_b128
// per plane), cut out by register selection (even offsets) or v_alignbit (odd).
// Workgroup = (tap-row group gi, split s): it runs over the (n, ho) rows of split s in
// 64-column stages -- dy[32 co][64] and x[4 rows][32 ci][80 columns] split into hi/mid/lo
// bf16 planes in LDS (81 KB, so two workgroups share a CU and cover each other's staging) --
// and writes its kw x 32 x 32 sums into slab s; wgrad_reduce_kernel adds the slabs in a fixed
// order (deterministic).
constexpr int CW_COLS = 64;
constexpr int CW_XP = 88;                  // x row pitch (bf16): 80 columns, 8 x odd
constexpr int CW_DP = 72;                  // dy row pitch (bf16): 64 columns, 8 x odd
constexpr int CW_XPL = 4 * 32 * CW_XP;     // bf16 per x plane
constexpr int CW_DPL = 32 * CW_DP;         // bf16 per dy plane

// 8 fp32 -> hi / mid / lo bf16 rows of 16 B (RNE casts, exact residuals)

// Partial sums of the bf16x6 weight-gradient kernels: one contiguous block per workgroup,
// partial[s][gi][co 32][w 4][b KW][ci 32] (tap row a = 4 gi + w) -- lane fr = ci, so every
// store instruction writes two whole 128-B runs; wgrad_reduce_x6_kernel sums the splits in
// order and scatters into dW[co][ci][a][b].  (The [co][ci][a][b] slab layout had each lane
// store to its own line: 2.6x the partial bytes in write traffic.)
                                           // (4 tap rows per group; NW rows: NW / 4 of them)
template <int KW, int NW = 4>
__device__ __forceinline__ void x6w_store_block(float* __restrict__ partial, int s, int G, int gi,
                                                int wave, bool active, int fr, int fh,
                                                const f32x16 (&acc)[KW]) {
  if (!active) return;   // rows a >= kh: never read by the reduce
  float* blk = partial + ((int64_t)s * G + gi) * (X6W_BLOCK / 4 * NW) * KW;
#pragma unroll
  for (int b = 0; b < KW; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = (r & 3) + 8 * (r >> 2) + 4 * fh;
      blk[((co * NW + wave) * KW + b) * 32 + fr] = acc[b][r];
    }
}

// dW[co][ci][a][b] = sum over the S splits (in order) of the blocks above; thread = one
// (gi, co, w, b, ci) element in block order (coalesced loads)
// co_amax / ci_amax (fp16x3 partials, else NULL): the sums are scaled by 2^(e_co + e_ci)
__global__ void wgrad_reduce_x6_kernel(const float* __restrict__ partial, int S, int G, int KW,
                                       int NW, ConvDims g, float* __restrict__ dw,
                                       const unsigned* __restrict__ co_amax,
                                       const unsigned* __restrict__ ci_amax) {
  const int64_t per = (int64_t)G * (X6W_BLOCK / 4 * NW) * KW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int ci = static_cast<int>(r % 32); r /= 32;
    const int b = static_cast<int>(r % KW); r /= KW;
    const int w = static_cast<int>(r % NW); r /= NW;
    const int co = static_cast<int>(r % 32);
    const int gi = static_cast<int>(r / 32);
    const int a = NW * gi + w;
    if (a >= g.kh || co >= g.co || ci >= g.ci) continue;
    float acc = 0.f;
#pragma unroll 8
    for (int s = 0; s < S; ++s) acc += partial[(int64_t)s * per + i];   // order kept
    if (co_amax != nullptr) acc = __builtin_ldexpf(acc, -(h3_exp(co_amax[co]) + h3_exp(ci_amax[ci])));
    dw[((int64_t)co * g.ci + ci) * g.kh * KW + a * KW + b] = acc;
  }
}

template <int KW, int OFF0>
__global__ __launch_bounds__(CW_T, 2) void conv_x6_wgrad_kernel(const float* __restrict__ dy,
                                                                 const float* __restrict__ x,
                                                                 float* __restrict__ partial,
                                                                 ConvDims g, int S) {
  __shared__ __attribute__((aligned(16))) unsigned short xs[3 * CW_XPL];
  __shared__ __attribute__((aligned(16))) unsigned short ds[3 * CW_DPL];
  constexpr int kOob = 0x7ffffff0;
  const int G = (g.kh + 3) / 4;
  // XCD-aware: the G tap-row groups of one split (the same x rows) get consecutive ids of
  // one XCD's run (blocks are dealt to the XCDs round-robin), so they share its L2
  int gi, s;
  {
    const int nwg = gridDim.x, o = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = o & 7;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (o >> 3);
    gi = id % G;
    s = id / G;
  }
  const int R = g.n * g.ho;
  const int r0 = static_cast<int>((int64_t)s * R / S);
  const int r1 = static_cast<int>((int64_t)(s + 1) * R / S);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = 4 * gi + wave;
  const bool active = a < g.kh;
  const int fr = lane & 31, fh = lane >> 5;
  const int nch = (g.wo + CW_COLS - 1) / CW_COLS;
  const int dplane = g.ho * g.wo, xplane = g.hi * g.wi;   // host: channel stacks < 2^31 B
  const int dco = tid >> 3, dseg = tid & 7;                 // dy staging: co, 8-column segment

  f32x16 acc[KW];
#pragma unroll
  for (int b = 0; b < KW; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  for (int row = r0; row < r1; ++row) {
    const int n = row / g.ho, ho = row - (row / g.ho) * g.ho;
    const __amdgpu_buffer_rsrc_t drs = conv_rsrc(dy + (int64_t)n * g.co * dplane, (int64_t)g.co * dplane);
    const __amdgpu_buffer_rsrc_t xrs = conv_rsrc(x + (int64_t)n * g.ci * xplane, (int64_t)g.ci * xplane);
    const int xr0 = ho * g.sh - g.ph + 4 * gi;
    for (int ch = 0; ch < nch; ++ch) {
      const int c0 = ch * CW_COLS;
      // one base offset per 8-column run; a column past either edge of its row (or a row
      // outside the input) loads from the out-of-range offset, i.e. zero
      float dv[8], xv[5][8];
      {
        const int cb = c0 + 8 * dseg;
        const int vo = dco < g.co ? (dco * dplane + ho * g.wo + cb) * 4 : kOob;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          dv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                drs, cb + i < g.wo ? vo + 4 * i : kOob, 0, 0));
        }
      }
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int id = tid + CW_T * u;
        const int j = id % 10, ci = (id / 10) & 31, w = id / 320;
        const int xr = xr0 + w;
        const bool ok = ci < g.ci && xr >= 0 && xr < g.hi && 4 * gi + w < g.kh;
        const int cb = c0 - 8 + 8 * j;
        const int vo = ok ? (ci * xplane + xr * g.wi + cb) * 4 : kOob;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool cok = cb + i >= 0 && cb + i < g.wi;
          xv[u][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                   xrs, cok ? vo + 4 * i : kOob, 0, 0));
        }
      }
      __syncthreads();   // every wave is done with the previous stage's fragments
      split_store8<3>(ds, CW_DPL, dco * CW_DP + 8 * dseg, dv);
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int id = tid + CW_T * u;
        const int j = id % 10, ci = (id / 10) & 31, w = id / 320;
        split_store8<3>(xs, CW_XPL, (w * 32 + ci) * CW_XP + 8 * j, xv[u]);
      }
      __syncthreads();
      if (active) {
#pragma unroll 1
        for (int kst = 0; kst < CW_COLS / 16; ++kst) {
          bf16x8 af[3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            af[pl] = *reinterpret_cast<const bf16x8*>(ds + pl * CW_DPL + fr * CW_DP + 16 * kst + 8 * fh);
          // one plane of x at a time (12 window registers): products with the lo, then
          // the mid, then the hi terms of x, each over the kw taps
#pragma unroll
          for (int pi = 0; pi < 3; ++pi) {
            const int pl = 2 - pi;
            unsigned wv[12];
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
              const u32x4 q = *reinterpret_cast<const u32x4*>(
                  xs + pl * CW_XPL + (wave * 32 + fr) * CW_XP + 8 * (2 * kst + fh + jj));
#pragma unroll
              for (int e = 0; e < 4; ++e) wv[4 * jj + e] = q[e];
            }
#pragma unroll
            for (int b = 0; b < KW; ++b) {
              const int o = b + OFF0;   // window offset of tap column b (compile time)
              u32x4 q;
#pragma unroll
              for (int e = 0; e < 4; ++e)
                q[e] = (o & 1) ? __builtin_amdgcn_alignbit(wv[(o + 1) / 2 + e], wv[(o - 1) / 2 + e], 16)
                               : wv[o / 2 + e];
              const bf16x8 bx = __builtin_bit_cast(bf16x8, q);
              // x term pl (0 hi, 1 mid, 2 lo) pairs with the dy terms i <= 2 - pl (the
              // products that carry fp32 weight), smaller terms first
#pragma unroll
              for (int i = 2 - pl; i >= 0; --i)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bx, acc[b], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  x6w_store_block<KW>(partial, s, G, gi, wave, active, fr, fh, acc);
}

// ---------------------------------------------------------------------------
// Sliding-window form of the bf16x6 weight gradient (default where conv_x6_wgrad_kernel
// applies and the height stride is <= 2).  Same workgroups (tap-row group gi of 4 rows, split
// s; 4 waves, one tap row each, kw accumulators) and the same per-tap MFMA step, but a split
// walks the (n, 32-column chunk, ho) rows with ho fastest: output row ho + 1's four x rows are
// row ho's moved down by sh, so each row stages only sh NEW x rows (plus its dy row) into a
// 6-slot ring (4 window rows + 2 incoming) -- 1.5 instead of 5 staging units of 8 values per
// thread -- while the MFMAs of row ho run on the other slots; one barrier per row.  Each x row
// is staged once per (group, chunk) instead of kh / sh times, and the G groups of a split run on
// one XCD (consecutive workgroup ids), so they share its L2 for x and dy.
constexpr int SW_XP = 56;                   // x slot row pitch (bf16): columns c0 - 8 .. c0 + 39;
                                            // 7 x 16 B (odd): ds_read_b128's 16-lane groups
                                            // hit 16 distinct 16-B bank slots (48 had 2-way
                                            // conflicts: 34 % of LDS cycles in SQ counters)
constexpr int SW_DP = 40;                   // dy row pitch (bf16): 32 columns, 5 x 16 B
constexpr int SW_XSL = 32 * SW_XP;          // bf16 per x slot (32 input channels)
constexpr int SW_DPL = 32 * SW_DP;          // bf16 per dy plane

// NW = 8: eight waves (tap rows) per group, one 512-thread workgroup per CU with a 10-slot ring
// (123 KB of LDS): G = 3 groups instead of 6 for conv2's 21 tap rows, so every x and dy row is
// staged -- and fetched -- half as often
// NPL 2: fp16x3 -- dy staged as fp16 hi / lo of dy 2^e_co (co_amax: max |dy| of each output
// channel over the batch), x as hi / lo of x 2^e_ci (ci_amax), three products per fragment pair;
// wgrad_reduce_x6_kernel undoes 2^-(e_co + e_ci) on the summed partials
// SWC = 64 (NW 8, fp16x3): 64-column row stages -- x slot pitch 88 (11 x 16 B), dy pitch 72
// (9 x 16 B), 80 x columns staged per 64 output columns instead of 48 per 32, half the stages
// and barriers per MFMA; 131 KB of LDS.  Staging units (x: 32 channels x 10 runs per row, dy: 32
// x 8): unit a = tid (waves 0-4 x row 0, waves 5-7 x row 1 units 0-191), unit b = waves 0-1 x
// row 1 units 192-319, waves 2-5 dy, waves 6-7 none (kinds wave-uniform)
template <int KW, int OFF0, int NW = 4, int NPL = 3, int SWC = SW_COLS>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void conv_x6_wgrad_sw_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
    ConvDims g, int S, const unsigned* __restrict__ co_amax, const unsigned* __restrict__ ci_amax) {
  static_assert(NW == 4 || NW == 8, "waves per group");
  static_assert(SWC == SW_COLS || (SWC == 64 && NW == 8 && NPL == 2), "64-column stages: NW 8, fp16x3");
  constexpr int RING = NW + 2;                // NW window rows + 2 incoming
  constexpr int XP = SWC == 64 ? 88 : SW_XP, DP = SWC == 64 ? 72 : SW_DP;
  constexpr int XSL = 32 * XP, DPL = 32 * DP;
  constexpr int XRUNS = (SWC + 16) / 8, DRUNS = SWC / 8;
  constexpr bool DY_IN_A = NW == 8 && SWC == SW_COLS;   // the dy waves' unit rides in va
  __shared__ __attribute__((aligned(16))) unsigned short xs[(SWC == 64 ? 2 : 3) * RING * XSL];
  __shared__ __attribute__((aligned(16))) unsigned short ds[2][(SWC == 64 ? 2 : 3) * DPL];
  constexpr int XPL = RING * XSL;
  constexpr int kOob = 0x7ffffff0;
  const int G = (g.kh + NW - 1) / NW;
  int gi, s;
  {
    const int nwg = gridDim.x, o = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = o & 7;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (o >> 3);
    gi = id % G;
    s = id / G;
  }
  const int nch = (g.wo + SWC - 1) / SWC;
  const int R = g.n * nch * g.ho;                           // host: < 2^31
  const int r0 = static_cast<int>((int64_t)s * R / S);
  const int r1 = static_cast<int>((int64_t)(s + 1) * R / S);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = NW * gi + wave;
  const bool active = a < g.kh;
  const int fr = lane & 31, fh = lane >> 5;
  const int dplane = g.ho * g.wo, xplane = g.hi * g.wi;   // host: channel stacks < 2^31 B
  const int wtop = NW * gi - g.ph;                          // window row 0 of output row 0
  // staging units (8 values each): 384 x units (incoming row r, channel, 8-column run j) and
  // 128 dy units (channel, run j).  NW = 4: thread t takes units t and t + 256 (unit kinds are
  // wave-uniform: waves 0-2 unit a row 0, wave 3 row 1; waves 0-1 unit b x row 1, waves 2-3
  // dy -- so the buffer resources stay scalar).  NW = 8: thread t takes unit t alone (waves
  // 0-2 x row 0, 3-5 x row 1, 6-7 dy; unit b unused)
  const int u1 = NW == 4 ? tid + 256 : tid;
  // (const initialisers, as in the 32-column form: assigning these inside if-constexpr branches
  // made hipcc 7.2 pack sc_a / sc_b into one register pair and apply them with v_pk_mul_f32
  // op_sel swapped -- wrong scales, test_conv_x6_wgrad_forms)
  constexpr bool W64 = SWC == 64;
  const int ta = W64 ? (wave < 5 ? tid : tid - 320) : (NW == 4 ? tid : (wave < 6 ? tid % 192 : 0));
  const int xr_a = W64 ? (wave >= 5 ? 1 : 0) : NW == 4 ? (wave == 3 ? 1 : 0) : (wave >= 3 ? 1 : 0);
  const int xc_a = W64 ? ta / XRUNS : NW == 4 ? (ta / 6) & 31 : ta / 6;
  const int xj_a = W64 ? ta % XRUNS : ta % 6;
  const bool a_is_x = W64 || NW == 4 || wave < 6;
  const bool b_is_x = W64 ? wave < 2 : NW == 4 && wave < 2;
  const bool b_is_dy = W64 ? (wave >= 2 && wave < 6) : NW == 4 ? wave >= 2 : wave >= 6;
  const int xc_b = W64 ? (192 + tid) / XRUNS : (u1 / 6) & 31;      // x unit: incoming row 1
  const int xj_b = W64 ? (192 + tid) % XRUNS : u1 % 6;
  const int dc_b = W64 ? (tid - 128) / DRUNS : (u1 - 384) >> 2;    // dy unit
  const int dj_b = W64 ? (tid - 128) % DRUNS : (u1 - 384) & 3;
  // fp16x3 staging scales of this thread's units (channels fixed for the whole launch)
  float sc_a = 1.f, sc_b = 1.f;
  if constexpr (NPL == 2) {
    if (a_is_x && xc_a < g.ci) sc_a = h3_scale(h3_exp(ci_amax[xc_a]));
    if (b_is_x && xc_b < g.ci) sc_b = h3_scale(h3_exp(ci_amax[xc_b]));
    if (b_is_dy && dc_b >= 0 && dc_b < g.co) {
      const float s = h3_scale(h3_exp(co_amax[dc_b]));
      if (DY_IN_A) sc_a = s; else sc_b = s;
    }
  }
  f32x16 acc[KW];
#pragma unroll
  for (int b = 0; b < KW; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  float va[8], vb[8];
  auto slot_of = [](int xr) { return ((xr % RING) + RING) % RING; };

  int row = r0;
  while (row < r1) {
    const int ho0 = row % g.ho, q = row / g.ho;
    const int ch = q % nch, n = q / nch;
    const int nrow = min(r1 - row, g.ho - ho0);              // rows of this (n, chunk) segment
    const int c0 = ch * SWC;
    const __amdgpu_buffer_rsrc_t drs = conv_rsrc(dy + (int64_t)n * g.co * dplane, (int64_t)g.co * dplane);
    const __amdgpu_buffer_rsrc_t xrs = conv_rsrc(x + (int64_t)n * g.ci * xplane, (int64_t)g.ci * xplane);
    // loads of x rows xr0 + r (r < nr; r = 0 unit a, r = 1 unit b) and, when hd >= 0, dy row hd
    auto load = [&](int xr0, int nr, int hd) {
      if (a_is_x) {
        const int xr = xr0 + xr_a, cb = c0 - 8 + 8 * xj_a;
        const bool ok = xr_a < nr && xc_a < g.ci && xr >= 0 && xr < g.hi;
        const int vo = ok ? (xc_a * xplane + xr * g.wi + cb) * 4 : kOob;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          va[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                xrs, (cb + i >= 0 && cb + i < g.wi) ? vo + 4 * i : kOob, 0, 0));
      }
      if (b_is_x) {
        const int xr = xr0 + 1, cb = c0 - 8 + 8 * xj_b;
        const bool ok = nr > 1 && xc_b < g.ci && xr >= 0 && xr < g.hi;
        const int vo = ok ? (xc_b * xplane + xr * g.wi + cb) * 4 : kOob;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          vb[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                xrs, (cb + i >= 0 && cb + i < g.wi) ? vo + 4 * i : kOob, 0, 0));
      } else if (b_is_dy) {
        // (NW = 8, 32 columns: the dy waves' unit goes in va, which they use for nothing else)
        const int cb = c0 + 8 * dj_b;
        const int vo = (hd >= 0 && dc_b < g.co) ? (dc_b * dplane + hd * g.wo + cb) * 4 : kOob;
        float* vd = DY_IN_A ? va : vb;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          vd[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                drs, cb + i < g.wo ? vo + 4 * i : kOob, 0, 0));
      }
    };
    auto store = [&](int xr0, int nr, int db) {
      if (a_is_x && xr_a < nr)
        split_store8<NPL>(xs, XPL, slot_of(xr0 + xr_a) * XSL + xc_a * XP + 8 * xj_a, va, sc_a);
      if (b_is_x) {
        if (nr > 1) split_store8<NPL>(xs, XPL, slot_of(xr0 + 1) * XSL + xc_b * XP + 8 * xj_b, vb, sc_b);
      } else if (b_is_dy && db >= 0) {
        split_store8<NPL>(ds[db], DPL, dc_b * DP + 8 * dj_b, DY_IN_A ? va : vb, DY_IN_A ? sc_a : sc_b);
      }
    };
    // segment start: every slot and dy buffer is free once all waves pass this barrier; the
    // NW window rows of ho0 go in NW / 2 passes (the first with ho0's dy row)
    const int xb0 = ho0 * g.sh + wtop;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NW / 2; ++p) {
      load(xb0 + 2 * p, 2, p == 0 ? ho0 : -1);
      store(xb0 + 2 * p, 2, p == 0 ? (ho0 & 1) : -1);
    }
    __syncthreads();
    for (int k = 0; k < nrow; ++k) {
      const int ho = ho0 + k;
      const bool more = k + 1 < nrow;
      const int xb = ho * g.sh + wtop;                      // window row 0 of this output row
      const int xin = xb + NW;                              // row ho + 1's incoming rows
      if (more) load(xin, g.sh, ho + 1);
      if (active) {
        const unsigned short* dsb = ds[ho & 1];
        const unsigned short* xsl = xs + slot_of(xb + wave) * XSL + fr * XP;
        // (SWC 64: unrolled by 2, 8 VGPRs spilled, 905 us in isolation; not unrolled, 1 spilled,
        // 943 us; fully unrolled, 10 spilled)
#pragma unroll(SWC == 64 ? 2 : SWC / 16)
        for (int kst = 0; kst < SWC / 16; ++kst) {
          bf16x8 af[3];
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl)
            af[pl] = *reinterpret_cast<const bf16x8*>(dsb + pl * DPL + fr * DP + 16 * kst + 8 * fh);
#pragma unroll
          for (int pi = 0; pi < NPL; ++pi) {
            const int pl = NPL - 1 - pi;
            unsigned wv[12];
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
              const u32x4 qv = *reinterpret_cast<const u32x4*>(xsl + pl * XPL + 8 * (2 * kst + fh + jj));
#pragma unroll
              for (int e = 0; e < 4; ++e) wv[4 * jj + e] = qv[e];
            }
#pragma unroll
            for (int b = 0; b < KW; ++b) {
              const int o = b + OFF0;
              u32x4 qb;
#pragma unroll
              for (int e = 0; e < 4; ++e)
                qb[e] = (o & 1) ? __builtin_amdgcn_alignbit(wv[(o + 1) / 2 + e], wv[(o - 1) / 2 + e], 16)
                                : wv[o / 2 + e];
              const bf16x8 bx = __builtin_bit_cast(bf16x8, qb);
#pragma unroll
              for (int i = NPL - 1 - pl; i >= 0; --i) {
                if constexpr (NPL == 2)
                  acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h(af[i]),
                                                                  as_h(bx),
                                                                  acc[b], 0, 0, 0);
                else
                  acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bx, acc[b], 0, 0, 0);
              }
            }
          }
        }
      }
      // the incoming slots held rows xb - 2, xb - 1 (read by row ho - 1, before the last
      // barrier); the other dy buffer likewise
      if (more) store(xin, g.sh, (ho + 1) & 1);
      __syncthreads();
    }
    row += nrow;
  }
  x6w_store_block<KW, NW>(partial, s, G, gi, wave, active, fr, fh, acc);
}

// ---------------------------------------------------------------------------
// bf16x6 dgrad with 4-row x 2-column fragments (default for <= 12 class tap rows and <= 12
// kernel columns: conv2's 11 x 11 class taps take 3 x 3 k-steps of 16 taps -- 144 tap slots
// for 121 -- instead of the 8-row fragments' 2 x 6 -- 192).  K order of k-step (row quad rq,
// column quad cq): lane half h takes tap rows 4 rq .. + 3 x tap columns 4 cq + 2 h, + 1
// (element 2 r + c).  The patch is stored as column PAIRS, [pair][row][2], twice -- pairs
// starting at even columns (E) and at odd columns (O) -- so a lane's 8 values are one 16-B run
// whatever the parity of its first column.  Pair pitch 24 bf16 (3 x 16 B) and the O copy 128 B
// off the E copy's bank phase: the 8 E and 8 O lanes of a b128 lane group hit 16 distinct
// 16-B bank slots.  Workgroup, waves, weight staging and epilogue as conv_x6_kernel's dgrad.
constexpr int CQ_PP = 2 * CQ_ROWS;                   // bf16 per column pair
constexpr int CQ_PAIRS = (CX_COLS + 11 + 1) / 2;     // pairs per copy (<= 12 kernel columns)
constexpr int CQ_OFFO = 3264;                        // O copy (bf16): 6528 B = 128 mod 256
constexpr int CQ_PPL = 6656;                         // bf16 per plane: 13312 B = 0 mod 256
constexpr int CQ_NK = 9;                             // 3 row quads x 3 column quads
constexpr int CQ_UNITS = 2 * CQ_PAIRS * 3;           // staging units (copy, pair, row quad)
static_assert(CQ_OFFO >= CQ_PAIRS * CQ_PP && CQ_OFFO + CQ_PAIRS * CQ_PP <= CQ_PPL, "patch plane");
static_assert(CQ_UNITS <= 2 * CX_T, "two staging units per thread");

// pre-split weight image [class][mb][co][plane][32 ci][CQ_COP]: k-step st, half h, element e
// (NPL 2: fp16 hi / lo planes of w 2^m_exp[ci])
template <int NPL = 3>
__global__ void conv_x6q_wimg_kernel(const float* __restrict__ w, ConvDims g,
                                     unsigned short* __restrict__ img,
                                     const int* __restrict__ m_exp, int flip_odd = 0) {
  const int M = g.ci, L = g.co;
  const int mbn = (M + 31) / 32;
  const int64_t per = (int64_t)32 * CQ_COP;
  const int64_t total = (int64_t)g.sh * mbn * L * per;
  const int KHW = g.kh * g.kw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int e = static_cast<int>(r % per); r /= per;
    const int l = static_cast<int>(r % L); r /= L;
    const int mb = static_cast<int>(r % mbn); r /= mbn;
    const int q = static_cast<int>(r);
    const int mm = e / CQ_COP, slot = e - mm * CQ_COP;
    const int m = mb * 32 + mm;
    float v = 0.f;
    if (slot < CQ_NK * 16 && m < M) {
      const int st = slot >> 4, h = (slot >> 3) & 1, x = slot & 7;
      const int a = 4 * (st / 3) + (x >> 1), b = 4 * (st % 3) + 2 * h + (x & 1);
      const int aq = class_taps(g, q);
      if (a < aq && b < g.kw)
        v = w[((int64_t)l * g.ci + m) * KHW + (q + g.sh * (aq - 1 - a)) * g.kw + (g.kw - 1 - b)];
    }
    // the second half of the k-steps (the kk = 1 waves' share) is stored negated: see the
    // dgrad kernel's epilogue (flip_odd: the odd loop channels instead, conv_h3_dgrad2r_kernel)
    if (flip_odd ? (l & 1) != 0 : slot >= ((CQ_NK + 1) / 2) * 16) v = -v;
    const float sc = NPL == 2 && m < M ? h3_scale(m_exp[m]) : 1.f;
    split_put<NPL>(img, ((((int64_t)q * mbn + mb) * L + l) * NPL) * per + e, per, v, sc);
  }
}

// DB: double-buffered patch and weight chunk (2 x 69 KB of LDS) -- channel l + 1 is staged
// into the other buffer right after the k-steps of channel l, one barrier per channel.  The
// patch gather offsets (and their bounds) are the same for every channel and are hoisted.
// NPL 2: fp16x3, scales as conv_x6_kernel's (e_n from the sample's max |dy|, m = ci)
// FL (fp16x3): the big products' chain restarts every input channel (see acf below).
// Sign split: the kk = 1 waves run on the negated weight image, so their chains hold -(their
// half), and the epilogue subtracts.  An MFMA rounds its addends' low bits toward -inf (bits
// below ~2^-31 of its largest operand, C included; profiles/r5n_mfma_rounding.txt), so every
// chain drifts negative; the negated half drifts the other way in the true sum and the two
// drifts cancel to their difference (5 vs 4 k-steps per channel) instead of adding.
template <bool DB, int NPL = 3, bool FL = true>
__global__ __launch_bounds__(CX_T, 1) void conv_x6q_dgrad_kernel(const float* __restrict__ dy,
                                                                 const unsigned short* __restrict__ img,
                                                                 float* __restrict__ dx, ConvDims g,
                                                                 int gx, int gy,
                                                                 const int* __restrict__ m_exp,
                                                                 const unsigned* __restrict__ n_amax) {
  constexpr int NB = DB ? 2 : 1;
  constexpr int WPL = 32 * CQ_COP;
  constexpr int wstride = NPL * WPL;
  __shared__ __attribute__((aligned(16))) unsigned short ps[NB * NPL * CQ_PPL];
  __shared__ __attribute__((aligned(16))) unsigned short ws[NB * wstride];
  const int M = g.ci, L = g.co;
  const int in_h = g.ho, in_w = g.wo, out_h = g.hi, out_w = g.wi;
  const int mbn = (M + 31) / 32;
  int bx, by, bz;
  xcd_tile(gx, gy, bx, by, bz);
  const int n = bz / mbn;
  const int mb = bz - n * mbn;
  const int m0 = mb * 32;
  const int c0 = bx * CX_COLS;
  int t = by, hq = 0, q;
  for (q = 0; q < g.sh; ++q) {
    hq = ((q - g.ph) % g.sh + g.sh) % g.sh;
    const int cnt = hq < g.hi ? (g.hi - 1 - hq) / g.sh + 1 : 0;
    if (t < cnt) break;
    t -= cnt;
  }
  const int A = class_taps(g, q);
  const int orow = hq + g.sh * t;
  const int prow0 = (orow + g.ph - q) / g.sh - (A - 1);
  const int pcol0 = c0 + g.pw - g.kw + 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cw = wave & 3, kk = wave >> 2;
  const int plane_in = in_h * in_w;
  const float* inn = dy + (int64_t)n * L * plane_in;
  const unsigned short* wimg = img + ((int64_t)q * mbn + mb) * L * wstride;
  constexpr int wchunks = wstride / 8;
  constexpr int WR = (wchunks + CX_T - 1) / CX_T;
  const int en = NPL == 2 ? h3_exp(n_amax[n]) : 0;
  const float nsc = h3_scale(en);

  // per-thread gather offsets (bytes; out-of-range elements read the buffer's zero tail)
  int goff[2][8];
  int soff[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int unit = tid + CX_T * u;
    const int cp = unit / (CQ_PAIRS * 3), rem = unit - cp * (CQ_PAIRS * 3);
    const int j = rem / 3, rq = rem - (rem / 3) * 3;
    const int col = pcol0 + 2 * j + cp;            // the pair's first column
    soff[u] = unit < CQ_UNITS ? cp * CQ_OFFO + j * CQ_PP + 8 * rq : -1;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const int a = 4 * rq + (x >> 1), ir = prow0 + a, ic = col + (x & 1);
      const bool ok = unit < CQ_UNITS && a < A && ir >= 0 && ir < in_h && ic >= 0 && ic < in_w;
      goff[u][x] = ok ? (ir * in_w + ic) * 4 : 0x7ffffff0;
    }
  }

  float rp[2][8];
  u32x4 rw[WR];
  auto load = [&](int l) {
    const __amdgpu_buffer_rsrc_t rs = conv_rsrc(inn + (int64_t)l * plane_in, plane_in);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int x = 0; x < 8; ++x)
        rp[u][x] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, goff[u][x], 0, 0));
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(wimg + (int64_t)l * wstride), (short)0, wstride * 2, 0x00020000);
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      const int i = tid + CX_T * r;
      rw[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                            wr, i < wchunks ? i * 16 : 0x7ffffff0, 0, 0));
    }
  };
  auto store = [&](int b) {
    unsigned short* pb = ps + b * (NPL * CQ_PPL);
    unsigned short* wb = ws + b * wstride;
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (soff[u] >= 0) split_store8<NPL>(pb, CQ_PPL, soff[u], rp[u], nsc);
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      const int i = tid + CX_T * r;
      if (i < wchunks) *reinterpret_cast<u32x4*>(wb + 8 * i) = rw[r];
    }
  };

  // acs: fp16x3's small products (cx_mma_h3s); acf: the big products' running sum.  The
  // big chain restarts from zero every input channel and is added into acf by the VALU
  // (RNE): an MFMA floors the addend bits below ~2^-31 of its largest operand, C included,
  // so a chain over all 32 channels drifted negative by ~160 x 2^-32 |C| at every position
  // -- the drift BatchNorm1's gradients (sums of dx over 1.3 M positions per channel)
  // collected, 5x the fp32 oracle's distance from fp64 (scripts/conv_block_stage_probe.py)
  f32x16 acc[2], acs[2], acf[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = acs[j][r] = acf[j][r] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;
  const bool active = orow < out_h && c0 + 64 * cw < out_w;
  constexpr int H0 = (CQ_NK + 1) / 2;

  load(0);
  store(0);
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const int cur = DB ? (l & 1) : 0;
    if (l + 1 < L) load(l + 1);
    if (active) {
      const unsigned short* pc = ps + cur * (NPL * CQ_PPL);
      const unsigned short* wc = ws + cur * wstride;
      auto kstep = [&](int st) {
        const int rq = st / 3, cq = st - (st / 3) * 3;
        bf16x8 af[3], bfr[2][3];
        const int aw = fr * CQ_COP + (st * 2 + fh) * 8;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) af[pl] = *reinterpret_cast<const bf16x8*>(wc + pl * WPL + aw);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int sc = 64 * cw + 32 * j + fr + 4 * cq + 2 * fh;   // first patch column
          const int ap = (sc & 1) * CQ_OFFO + (sc >> 1) * CQ_PP + 8 * rq;
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl)
            bfr[j][pl] = *reinterpret_cast<const bf16x8*>(pc + pl * CQ_PPL + ap);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (NPL == 2) cx_mma_h3s(af, bfr[j], acc[j], acs[j]);
          else acc[j] = cx_mma<NPL>(af, bfr[j], acc[j]);
        }
      };
      if (kk == 0) {
#pragma unroll
        for (int st = 0; st < H0; ++st) kstep(st);
      } else {
#pragma unroll
        for (int st = H0; st < CQ_NK; ++st) kstep(st);
      }
      if constexpr (NPL == 2 && FL) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acf[j] += acc[j];
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        }
      }
    }
    if (DB) {
      // the other buffer was last read in channel l - 1, before the previous barrier
      if (l + 1 < L) store(cur ^ 1);
      __syncthreads();
    } else {
      __syncthreads();
      if (l + 1 < L) {
        store(0);
        __syncthreads();
      }
    }
  }
  if constexpr (NPL == 2) {
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j] = FL ? acf[j] + acs[j] : acc[j] + acs[j];
  }
  // the two k halves meet in LDS (the patch area): half 1 writes, half 0 adds (fixed order)
  float* red = reinterpret_cast<float*>(ps);
  if (kk == 1) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((cw * 2 + j) * 16 + r) * 64 + lane] = acc[j][r];
  }
  __syncthreads();
  if (kk == 1 || !active) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = c0 + 64 * cw + 32 * j + fr;
    if (col >= out_w) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      if (m < M) {
        float v = acc[j][r] - red[((cw * 2 + j) * 16 + r) * 64 + lane];   // sign split
        if (NPL == 2) v = __builtin_ldexpf(v, -(m_exp[m] + en));
        dx[(((int64_t)n * M + m) * out_h + orow) * out_w + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// conv2 dgrad on fp16x3, two dx rows per workgroup: rows t and t + 4 of one stride class (dx
// rows hq + sh t) read dy rows 4 apart -- exactly one row quad of the 4 x 2 fragments -- so ONE
// column-pair patch of 16 dy rows serves both (row t's B fragments are quads 0..2, row t + 4's
// quads 1..3) and both multiply the SAME weight fragments.  Per loop channel a workgroup then
// stages 16 patch rows and one weight image for two dx rows (conv_x6q_dgrad_kernel: 12 rows and
// one image for one row).  Waves: 8 x 32 columns, all 9 k-steps of both rows.  Both MFMA chains
// (big and small products) restart every channel and are folded into a VALU sum (RNE), so no
// chain is longer than 9 MFMAs; and the k-half sign split becomes a split by channel parity: odd
// channels run on the negated weight image and are subtracted, so the MFMAs' floor of low
// addend bits drifts the even and the odd channels' terms in opposite directions.  Pair pitch 40 fp16
// (5 x 16 B, odd) and the O copy 128 B off the E copy's bank phase keep the b128 fragment reads
// conflict-free as in conv_x6q_dgrad_kernel.
constexpr int C2Q_ROWS = 16;                          // patch rows: 12 class taps + one quad
constexpr int C2Q_PP = 40;                            // fp16 per column pair
constexpr int C2Q_OFFO = 5440;                        // O copy: 10880 B = 128 mod 256
constexpr int C2Q_PPL = 10880;                        // fp16 per plane: 21760 B = 0 mod 256
constexpr int C2Q_UNITS = 2 * CQ_PAIRS * (C2Q_ROWS / 4);   // (copy, pair, row quad) units
constexpr int C2Q_PU = (C2Q_UNITS + CX_T - 1) / CX_T;
static_assert(C2Q_OFFO >= CQ_PAIRS * C2Q_PP && C2Q_OFFO + CQ_PAIRS * C2Q_PP <= C2Q_PPL, "patch plane");

__global__ __launch_bounds__(CX_T, 1) void conv_h3_dgrad2r_kernel(
    const float* __restrict__ dy, const unsigned short* __restrict__ img, float* __restrict__ dx,
    ConvDims g, int gx, int gy, const int* __restrict__ m_exp,
    const unsigned* __restrict__ n_amax) {
  constexpr int WPL = 32 * CQ_COP;
  constexpr int wstride = 2 * WPL;
  __shared__ __attribute__((aligned(16))) unsigned short ps[2 * 2 * C2Q_PPL];
  __shared__ __attribute__((aligned(16))) unsigned short ws[2 * wstride];
  const int M = g.ci, L = g.co;
  const int in_h = g.ho, in_w = g.wo, out_h = g.hi, out_w = g.wi;
  const int mbn = (M + 31) / 32;
  int bx, by, bz;
  xcd_tile(gx, gy, bx, by, bz);
  const int n = bz / mbn;
  const int mb = bz - n * mbn;
  const int m0 = mb * 32;
  const int c0 = bx * CX_COLS;
  // (class q, row pair) of this workgroup: rows t and t + 4 with t = 8 b + j, j < 4
  int pr = by, hq = 0, q, cnt = 0;
  for (q = 0; q < g.sh; ++q) {
    hq = ((q - g.ph) % g.sh + g.sh) % g.sh;
    cnt = hq < g.hi ? (g.hi - 1 - hq) / g.sh + 1 : 0;
    const int pairs = 4 * (cnt / 8) + min(4, cnt % 8);
    if (pr < pairs) break;
    pr -= pairs;
  }
  const int t = 8 * (pr >> 2) + (pr & 3);
  const int A = class_taps(g, q);
  const int orow = hq + g.sh * t;                      // and orow + 4 sh (class row t + 4)
  const bool second = t + 4 < cnt;
  const int prow0 = (orow + g.ph - q) / g.sh - (A - 1);
  const int pcol0 = c0 + g.pw - g.kw + 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plane_in = in_h * in_w;
  const float* inn = dy + (int64_t)n * L * plane_in;
  const unsigned short* wimg = img + ((int64_t)q * mbn + mb) * L * wstride;
  constexpr int wchunks = wstride / 8;
  constexpr int WR = (wchunks + CX_T - 1) / CX_T;
  const int en = h3_exp(n_amax[n]);
  const float nsc = h3_scale(en);

  int goff[C2Q_PU][8];
  int soff[C2Q_PU];
#pragma unroll
  for (int u = 0; u < C2Q_PU; ++u) {
    const int unit = tid + CX_T * u;
    const int cp = unit / (CQ_PAIRS * 4), rem = unit - cp * (CQ_PAIRS * 4);
    const int j = rem >> 2, rq = rem & 3;
    const int col = pcol0 + 2 * j + cp;
    soff[u] = unit < C2Q_UNITS ? cp * C2Q_OFFO + j * C2Q_PP + 8 * rq : -1;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const int a = 4 * rq + (x >> 1), ir = prow0 + a, ic = col + (x & 1);
      const bool ok = unit < C2Q_UNITS && a < A + 4 && ir >= 0 && ir < in_h && ic >= 0 && ic < in_w;
      goff[u][x] = ok ? (ir * in_w + ic) * 4 : 0x7ffffff0;
    }
  }

  float rp[C2Q_PU][8];
  u32x4 rw[WR];
  auto load = [&](int l) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t rs = conv_rsrc(inn + (int64_t)l * plane_in, plane_in);
#pragma unroll
    for (int u = 0; u < C2Q_PU; ++u)
#pragma unroll
      for (int x = 0; x < 8; ++x)
        rp[u][x] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, goff[u][x], 0, 0));
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(wimg + (int64_t)l * wstride), (short)0, wstride * 2, 0x00020000);
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      const int i = tid + CX_T * r;
      rw[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                            wr, i < wchunks ? i * 16 : 0x7ffffff0, 0, 0));
    }
  };
  auto store = [&](int b) __attribute__((always_inline)) {
    unsigned short* pb = ps + b * (2 * C2Q_PPL);
    unsigned short* wb = ws + b * wstride;
#pragma unroll
    for (int u = 0; u < C2Q_PU; ++u)
      if (soff[u] >= 0) split_store8<2>(pb, C2Q_PPL, soff[u], rp[u], nsc);
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      const int i = tid + CX_T * r;
      if (i < wchunks) *reinterpret_cast<u32x4*>(wb + 8 * i) = rw[r];
    }
  };

  f32x16 acc[2], acs[2], acf[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = acs[j][r] = acf[j][r] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;
  const bool active = c0 + 32 * wave < out_w;

  load(0);
  store(0);
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const int cur = l & 1;
    if (l + 1 < L) load(l + 1);
    if (active) {
      const unsigned short* pc = ps + cur * (2 * C2Q_PPL);
      const unsigned short* wc = ws + cur * wstride;
#pragma unroll
      for (int st = 0; st < CQ_NK; ++st) {
        const int rq = st / 3, cq = st - (st / 3) * 3;
        bf16x8 af[3], b0[3], b1[3];
        const int aw = fr * CQ_COP + (st * 2 + fh) * 8;
        const int sc = 32 * wave + fr + 4 * cq + 2 * fh;   // the lane's first patch column
        const int ap = (sc & 1) * C2Q_OFFO + (sc >> 1) * C2Q_PP + 8 * rq;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          af[pl] = *reinterpret_cast<const bf16x8*>(wc + pl * WPL + aw);
          b0[pl] = *reinterpret_cast<const bf16x8*>(pc + pl * C2Q_PPL + ap);
          b1[pl] = *reinterpret_cast<const bf16x8*>(pc + pl * C2Q_PPL + ap + 8);
        }
        cx_mma_h3s(af, b0, acc[0], acs[0]);
        cx_mma_h3s(af, b1, acc[1], acs[1]);
      }
      // both chains restart every channel; odd channels ran on negated weights, so their
      // chains hold -(their sum) and drift the other way in the true sum
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (l & 1) acf[j] -= acc[j] + acs[j];
        else acf[j] += acc[j] + acs[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = acs[j][r] = 0.f;
      }
    }
    // the other buffer was last read in channel l - 1, before the previous barrier
    if (l + 1 < L) store(cur ^ 1);
    __syncthreads();
  }
  if (!active) return;
  const int col = c0 + 32 * wave + fr;
  if (col >= out_w) return;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    if (rr == 1 && !second) continue;
    const int row = orow + 4 * g.sh * rr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      if (m < M) {
        const float v = __builtin_ldexpf(acf[rr][r], -(m_exp[m] + en));
        dx[(((int64_t)n * M + m) * out_h + row) * out_w + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The launches.  Every number comes from the plan (conv_host.h).
template <typename T>
static inline T* ws_at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }
static inline dim3 wimg_grid(const ConvPlan& p) { return dim3(std::min(cdiv(p.img, 256), 2048)); }

// conv_x6_kernel<DGRAD, NGA, NBP, PU, SW, RCH, DB, NPL> on the plan's grid, its weight image first
template <bool DGRAD, int NGA, int NBP, int PU, int SW, bool RCH, bool DB = false, int NPL = 3>
static void launch_x6(const ConvPlan& p, const ConvDims& g, const float* in, const float* w,
                      const float* bias, float* out, const int* out_lens, unsigned short* img,
                      const int* m_exp, const unsigned* n_amax, hipStream_t st) {
  const CxGeom c = cx_geom(g, DGRAD);
  hipLaunchKernelGGL((conv_x6_wimg_kernel<DGRAD, NPL>), wimg_grid(p), dim3(256), 0, st, w, g, c, img,
                     m_exp);
  hipLaunchKernelGGL((conv_x6_kernel<DGRAD, NGA, NBP, PU, SW, RCH, DB, NPL>),
                     dim3(static_cast<unsigned>(p.grid)), dim3(CX_T), 0, st, in, img, bias, out, g,
                     out_lens, c, p.gx, p.gy, m_exp, n_amax);
}

ds2_status_t launch_conv_split(const ConvPlan& p, const ConvDims& g, const float* in,
                               const float* w, const float* bias, float* out, const int* out_lens,
                               void* ws, hipStream_t st) {
  const bool dgrad = p.rung >= DS2_CONV_DG_H3_2R;
  unsigned short* img = static_cast<unsigned short*>(ws);
  const dim3 grid(static_cast<unsigned>(p.grid)), cxt(CX_T);
  int* m_exp = nullptr;
  unsigned* n_amax = nullptr;
  if (p.h3) {
    // the fp16x3 scales: m_exp (per output row m of the implicit GEMM) and n_amax (per sample
    // of the staged input `in`, [n][L][plane_in])
    const int64_t per = dgrad ? (int64_t)g.co * g.ho * g.wo : (int64_t)g.ci * g.hi * g.wi;
    m_exp = ws_at<int>(ws, p.m_exp);
    n_amax = ws_at<unsigned>(ws, p.n_amax);
    if (dgrad)
      hipLaunchKernelGGL(conv_h3_wexp_kernel<true>, dim3(g.ci), dim3(256), 0, st, w, g, m_exp);
    else
      hipLaunchKernelGGL(conv_h3_wexp_kernel<false>, dim3(g.co), dim3(256), 0, st, w, g, m_exp);
    (void)hipMemsetAsync(n_amax, 0, (size_t)g.n * 4, st);
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(cdiv(per, 8192), cdiv(2048, g.n)));
    hipLaunchKernelGGL(conv_h3_samax_kernel, dim3(static_cast<unsigned>(chunks), g.n), dim3(256), 0,
                       st, in, per, n_amax);
  }
  switch (p.rung) {
    case DS2_CONV_FWD_H3_2R:   // the image's odd loop channels negated (flip_odd 1)
      hipLaunchKernelGGL((conv_x6_wimg_kernel<false, 2>), wimg_grid(p), dim3(256), 0, st, w, g,
                         cx_geom(g, false), img, m_exp, 1);
      hipLaunchKernelGGL(conv_h3_fwd2r_kernel, grid, cxt, 0, st, in, img, bias, out, g, out_lens, p.gx,
                         p.gy, m_exp, n_amax);
      break;
    case DS2_CONV_FWD_H3_1R:
      launch_x6<false, 3, 6, 2, 1, false, true, 2>(p, g, in, w, bias, out, out_lens, img, m_exp, n_amax, st);
      break;
    case DS2_CONV_FWD_X6_DB:
      launch_x6<false, 3, 6, 2, 1, false, true>(p, g, in, w, bias, out, out_lens, img, nullptr, nullptr, st);
      break;
    case DS2_CONV_FWD_X6:
      launch_x6<false, 0, 0, 3, 0, true>(p, g, in, w, bias, out, out_lens, img, nullptr, nullptr, st);
      break;
    case DS2_CONV_DG_H3_2R:    // odd loop channels negated
      hipLaunchKernelGGL(conv_x6q_wimg_kernel<2>, wimg_grid(p), dim3(256), 0, st, w, g, img, m_exp, 1);
      hipLaunchKernelGGL(conv_h3_dgrad2r_kernel, grid, cxt, 0, st, in, img, out, g, p.gx, p.gy, m_exp,
                         n_amax);
      break;
    case DS2_CONV_DG_H3_Q:
    case DS2_CONV_DG_H3_Q_NOFLUSH:
      hipLaunchKernelGGL(conv_x6q_wimg_kernel<2>, wimg_grid(p), dim3(256), 0, st, w, g, img, m_exp);
      hipLaunchKernelGGL((p.rung == DS2_CONV_DG_H3_Q ? conv_x6q_dgrad_kernel<true, 2, true>
                                                     : conv_x6q_dgrad_kernel<true, 2, false>),
                         grid, cxt, 0, st, in, img, out, g, p.gx, p.gy, m_exp, n_amax);
      break;
    case DS2_CONV_DG_X6_Q:
      hipLaunchKernelGGL(conv_x6q_wimg_kernel<3>, wimg_grid(p), dim3(256), 0, st, w, g, img, nullptr);
      hipLaunchKernelGGL((conv_x6q_dgrad_kernel<true, 3>), grid, cxt, 0, st, in, img, out, g, p.gx, p.gy,
                         nullptr, nullptr);
      break;
    case DS2_CONV_DG_X6_26:    // 8-row fragments, compile-time 2 x 6
      launch_x6<true, 2, 6, 2, 1, false>(p, g, in, w, nullptr, out, nullptr, img, nullptr, nullptr, st);
      break;
    case DS2_CONV_DG_X6:
      launch_x6<true, 0, 0, 3, 0, true>(p, g, in, w, nullptr, out, nullptr, img, nullptr, nullptr, st);
      break;
    default:
      return DS2_INVALID_VALUE;
  }
  return launch_status(dgrad ? "ds2_conv2d_dgrad" : "ds2_conv2d_fwd");
}

ds2_status_t launch_conv_split_wgrad(const ConvPlan& p, const ConvDims& g, const float* dy,
                                     const float* x, float* dw, void* ws, hipStream_t st) {
  float* partial = static_cast<float*>(ws);
  const int nw = p.a, G = p.b;
  const dim3 grid(static_cast<unsigned>(p.grid));
  unsigned* co_am = nullptr;   // fp16x3 channel maxima
  unsigned* ci_am = nullptr;
  if (p.h3) {
    co_am = ws_at<unsigned>(ws, p.co_amax);
    ci_am = ws_at<unsigned>(ws, p.ci_amax);
    if (hipMemsetAsync(co_am, 0, ((size_t)g.co + g.ci) * 4, st) != hipSuccess)
      return launch_status("ds2_conv2d_wgrad");
    const int64_t dpl = (int64_t)g.ho * g.wo, xpl = (int64_t)g.hi * g.wi;
    const int cd = static_cast<int>(std::min<int64_t>(64, cdiv((int64_t)g.n * dpl, 16384)));
    const int cx = static_cast<int>(std::min<int64_t>(64, cdiv((int64_t)g.n * xpl, 16384)));
    hipLaunchKernelGGL(conv_h3_chamax_kernel, dim3(cd, g.co), dim3(256), 0, st, dy, g.n, g.co, dpl,
                       co_am);
    hipLaunchKernelGGL(conv_h3_chamax_kernel, dim3(cx, g.ci), dim3(256), 0, st, x, g.n, g.ci, xpl,
                       ci_am);
  }
  if (p.rung == DS2_CONV_WG_X6_ROW)
    hipLaunchKernelGGL((conv_x6_wgrad_kernel<11, 3>), grid, dim3(CW_T), 0, st, dy, x, partial, g,
                       p.splits);
  else   // the 64-column form is opt-in: less HBM traffic, 8 VGPRs spilled, 3-5 % slower
    hipLaunchKernelGGL((p.rung == DS2_CONV_WG_H3_SW64   ? conv_x6_wgrad_sw_kernel<11, 3, 8, 2, 64>
                        : p.rung == DS2_CONV_WG_H3_SW32 ? conv_x6_wgrad_sw_kernel<11, 3, 8, 2>
                                                        : conv_x6_wgrad_sw_kernel<11, 3, 8>),
                       grid, dim3(512), 0, st, dy, x, partial, g, p.splits, co_am, ci_am);
  const int64_t blk = (int64_t)G * (X6W_BLOCK / 4 * nw) * g.kw;
  const int xg = static_cast<int>(std::min<int64_t>(cdiv(blk, 256), 2048));
  hipLaunchKernelGGL(wgrad_reduce_x6_kernel, dim3(xg), dim3(256), 0, st, partial, p.splits, G, g.kw, nw,
                     g, dw, co_am, ci_am);
  return launch_status("ds2_conv2d_wgrad");
}

}  // namespace ds2
