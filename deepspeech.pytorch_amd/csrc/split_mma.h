// Split-operand arithmetic: fp32-class products on the fp16 / bf16 matrix cores.  The one
// statement of the splits and of the product order for every kernel that uses them (gemm.hip,
// bgemm.hip, conv_split.hip, conv1d.hip, gru_split.hip, gru_xl.hip, lstm.hip); the CPU error
// model in tests/gemm_common.py (h3_exp, h3_split, h3_bound) restates this file.  Device inline
// functions and typedefs only: no kernel, no host code.
//
//   fp16x3: a row scaled by 2^e (h3_exp) splits into hi = f16(x 2^e), lo = f16(x 2^e - hi);
//           a.b = lo.hi + hi.lo + hi.hi (lo.lo, below 2^-22 |a b|, dropped).
//   bf16x6: x splits into hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid);
//           a.b = mid.mid + lo.hi + hi.lo + mid.hi + hi.mid + hi.hi (mid.lo, lo.mid, lo.lo,
//           each below 2^-24 |a b|, dropped).
// Every conversion rounds to nearest even, every residual is exact in fp32, and every product
// is exact in the fp32 accumulator, so a result carries fp32 rounding only.
//
// Product order.  The small products go first.  The matrix cores sum the products and C of one
// instruction exactly and round once (RNE), but they floor (truncate toward -inf) each addend's
// bits below ~2^-31 of the instruction's largest operand, C included (scripts/mfma_rounding.hip,
// profiles/r5n_mfma_rounding.txt).  A small product chained beside hi.hi or a large C loses its
// low bits downward: ~1e-7 relative per result, noise per element but a NEGATIVE bias in sums
// over many outputs (the conv block's BatchNorm parameter gradients: 1.3 M nearly cancelling
// terms; the recurrences' bias gradients).  Kernels whose outputs feed such sums keep the small
// products in a chain of their own (mma3h2: their C stays ~2^-11 of the big one's, so they keep
// every bit) and join the chains by a VALU add (RNE): the conv2 forward and dgrad, the backward
// recurrences.  The forward recurrences, the GEMMs and conv1d, whose results are not summed up,
// keep one chain (mma3h): splitting it cost the GRU forward 1.95 -> 2.32 ms per launch (the
// join is a VALU add on the critical path of every hand-off step).
#pragma once

#include "common.h"

namespace ds2 {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// --- fp16x3 row scales -------------------------------------------------------------------
// amax: the bit pattern of max |x| over a logical row (non-negative floats order as unsigned).
// The row is staged as x 2^e, e = 14 - floor(log2 amax), so its largest element lies in
// [2^14, 2^15) (fp16 max 65504) and its fp16 (hi, lo) split keeps 22 bits for every element
// within 2^17 of the row max; a zero, inf or NaN row max keeps e = 0.
__device__ __forceinline__ int h3_exp(unsigned amax) {
  const int E = (int)(amax >> 23);                 // biased exponent (sign bit is 0)
  if (amax == 0u || E >= 255) return 0;
  int e = 14 - ((E == 0 ? 1 : E) - 127);
  return e > 127 ? 127 : e;                        // 2^e stays a normal float
}
__device__ __forceinline__ float h3_scale(int e) { return __builtin_bit_cast(float, (e + 127) << 23); }
__device__ __forceinline__ int h3_row_exp(float m) { return h3_exp(__float_as_uint(m)); }

// --- splits ------------------------------------------------------------------------------
// two fp32 -> (hi, mid, lo) bf16 pairs: one v_cvt_pk_bf16_f32 (RNE) per term pair, the
// residuals exact in fp32 (bit-identical to per-element casts, half the instructions)
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& h, unsigned& m,
                                            unsigned& l) {
  h = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
  const float r0 = x0 - __builtin_bit_cast(float, h << 16);
  const float r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
  const float l0 = r0 - __builtin_bit_cast(float, m << 16);
  const float l1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{l0, l1}, bf16x2));
}

// The store form (the GEMMs' and convolutions' LDS staging): 8 fp32 -> NPL rows of 16 B at
// s + at, + plane, + 2 plane.  NPL 3: the bf16 hi / mid / lo planes; NPL 1: the bf16 (RNE)
// rounding alone (the bf16-operand GEMM); NPL 2: the fp16 hi / lo planes of v sc (sc = 2^e, the
// operand row's scale)
template <int NPL = 3>
__device__ __forceinline__ void split_store8(unsigned short* __restrict__ s, int plane, int at,
                                             const float* v, float sc = 1.f) {
  if constexpr (NPL == 2) {
    u32x4 h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 x = f32x2{v[2 * j], v[2 * j + 1]} * sc;
      const f16x2 hh = __builtin_convertvector(x, f16x2);
      const f32x2 r = x - __builtin_convertvector(hh, f32x2);
      h[j] = __builtin_bit_cast(unsigned, hh);
      l[j] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
    }
    *reinterpret_cast<u32x4*>(s + at) = h;
    *reinterpret_cast<u32x4*>(s + plane + at) = l;
  } else if constexpr (NPL == 1) {
    u32x4 h;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      h[j] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v[2 * j], v[2 * j + 1]}, bf16x2));
    *reinterpret_cast<u32x4*>(s + at) = h;
  } else {
    u32x4 h, m, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned a, b, c;
#if defined(DS2_X6_ABL) && DS2_X6_ABL == 3
      // gemm.hip's ablation build: the hi term only (no residual splits)
      a = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v[2 * j], v[2 * j + 1]}, bf16x2));
      b = a;
      c = a;
#else
      split3_pair(v[2 * j], v[2 * j + 1], a, b, c);
#endif
      h[j] = a;
      m[j] = b;
      l[j] = c;
    }
    *reinterpret_cast<u32x4*>(s + at) = h;
    *reinterpret_cast<u32x4*>(s + plane + at) = m;
    *reinterpret_cast<u32x4*>(s + 2 * plane + at) = l;
  }
}

// The register forms (the recurrences, whose operands never pass through LDS planes): 8 fp32
// values, MFMA k slots 0..3 from a and 4..7 from b.  fp16x3 there (the default since round 5):
// h (|h| <= 1) takes the fixed scale 2^14, each W_hh row (gate, unit) its own (h3_row_exp),
// found at kernel start; half the MFMAs of the bf16x6 form and two operand terms for three.
struct Duo {
  f16x8 hi, lo;
};
struct Tri {
  bf16x8 hi, mid, lo;
};

// times sc -> fp16 (hi, lo)
__device__ __forceinline__ Duo split2h(const f32x4 a, const f32x4 b, float sc) {
  Duo t;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 x = (j < 2 ? f32x2{a[2 * j], a[2 * j + 1]} : f32x2{b[2 * j - 4], b[2 * j - 3]}) * sc;
    const f16x2 h = __builtin_convertvector(x, f16x2);
    const f16x2 l = __builtin_convertvector(x - __builtin_convertvector(h, f32x2), f16x2);
    t.hi[2 * j] = h[0];
    t.hi[2 * j + 1] = h[1];
    t.lo[2 * j] = l[0];
    t.lo[2 * j + 1] = l[1];
  }
  return t;
}

// -> three bf16 terms, per-element casts (the W_hh splits at kernel start)
__device__ __forceinline__ Tri split3(const f32x4 a, const f32x4 b) {
  Tri t;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = j < 4 ? a[j] : b[j - 4];
    const __bf16 h = (__bf16)v;
    const float r1 = v - (float)h;
    const __bf16 m = (__bf16)r1;
    const float r2 = r1 - (float)m;
    t.hi[j] = h;
    t.mid[j] = m;
    t.lo[j] = (__bf16)r2;
  }
  return t;
}

// 4 fp32 -> their (hi, mid) bf16 terms packed as one 16-B run {hi01, hi23, mid01, mid23} and
// their lo terms as one 8-B run (the terms split3 forms): a producer's pre-split hand-off tile
__device__ __forceinline__ void split_pk4(const f32x4 v, u32x4& hm, u32x2& lo) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    unsigned h, m, l;
    split3_pair(v[2 * q], v[2 * q + 1], h, m, l);
    hm[q] = h;
    hm[2 + q] = m;
    lo[q] = l;
  }
}

// the Tri of a 32-k pair from two pre-split tiles' runs (slots 0..3 tile a, 4..7 tile b)
__device__ __forceinline__ Tri tri_of(const u32x4 ha, const u32x2 la, const u32x4 hb, const u32x2 lb) {
  Tri t;
  t.hi = __builtin_bit_cast(bf16x8, u32x4{ha[0], ha[1], hb[0], hb[1]});
  t.mid = __builtin_bit_cast(bf16x8, u32x4{ha[2], ha[3], hb[2], hb[3]});
  t.lo = __builtin_bit_cast(bf16x8, u32x4{la[0], la[1], lb[0], lb[1]});
  return t;
}

// The scalar form (weight images, written once per call): one value's NPL terms, `per` apart
// from img[base]
template <int NPL>
__device__ __forceinline__ void split_put(unsigned short* __restrict__ img, int64_t base,
                                          int64_t per, float v, float sc) {
  if constexpr (NPL == 2) {
    const float x = v * sc;
    const _Float16 hb = (_Float16)x;
    img[base] = __builtin_bit_cast(unsigned short, hb);
    img[base + per] = __builtin_bit_cast(unsigned short, (_Float16)(x - (float)hb));
  } else {
    const __bf16 hb = (__bf16)v;
    const float r1 = v - (float)hb;
    const __bf16 mbf = (__bf16)r1;
    const __bf16 lb = (__bf16)(r1 - (float)mbf);
    img[base] = __builtin_bit_cast(unsigned short, hb);
    img[base + per] = __builtin_bit_cast(unsigned short, mbf);
    img[base + 2 * per] = __builtin_bit_cast(unsigned short, lb);
  }
}

// --- product groups ----------------------------------------------------------------------
// One MFMA; the accumulator picks the shape: f32x4 16x16x32, f32x16 32x32x16.
__device__ __forceinline__ f32x4 mfma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

// c + a.b, bf16x6: six products, small terms first
template <typename C>
__device__ __forceinline__ C mma6(bf16x8 ah, bf16x8 am, bf16x8 al, bf16x8 bh, bf16x8 bm, bf16x8 bl, C c) {
  c = mfma(am, bm, c);
  c = mfma(al, bh, c);
  c = mfma(ah, bl, c);
  c = mfma(am, bh, c);
  c = mfma(ah, bm, c);
  return mfma(ah, bh, c);
}
template <typename C>
__device__ __forceinline__ C mma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], C c) {
  return mma6(a[0], a[1], a[2], b[0], b[1], b[2], c);
}
__device__ __forceinline__ f32x4 mma6(const Tri& a, const Tri& b, f32x4 c) {
  return mma6(a.hi, a.mid, a.lo, b.hi, b.mid, b.lo, c);
}

// c + a.b, fp16x3 in one chain (small terms first)
template <typename C>
__device__ __forceinline__ C mma3h(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, C c) {
  c = mfma(al, bh, c);
  c = mfma(ah, bl, c);
  return mfma(ah, bh, c);
}
__device__ __forceinline__ f32x4 mma3h(const Duo& a, const Duo& b, f32x4 c) {
  return mma3h(a.hi, a.lo, b.hi, b.lo, c);
}

// fp16x3 in two chains: big += hi.hi, small += lo.hi + hi.lo (see the top of this file)
template <typename C>
__device__ __forceinline__ void mma3h2(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, C& big, C& small) {
  small = mfma(al, bh, small);
  small = mfma(ah, bl, small);
  big = mfma(ah, bh, big);
}

}  // namespace ds2
