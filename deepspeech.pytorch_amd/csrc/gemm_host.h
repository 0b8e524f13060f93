// Host side of the GEMM family (gemm.hip, bgemm.hip): the work decode host and device share,
// the tile sizes the planner uses, the work plan, and ONE selection function per call --
// which kernel runs (the rung), on which plan, with which flags and how much workspace.
// ds2_sgemm*, ds2_sgemm_bf16_ws, ds2_bgemm_nt, the workspace queries and ds2_test_sgemm_plan
// all go through gemm_select; nothing else decides.  DESIGN.md "GEMM dispatch" has the table.
//
// Plain C++ apart from the __host__ __device__ markers of the decode: it compiles without
// the HIP runtime (a stand-alone host program can include it, e.g. under a sanitizer).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/ds2hip.h"
#include "../../include/ds2hip_test.h"

#if defined(__HIPCC__)
#define DS2_HD __host__ __device__ __forceinline__
#else
#define DS2_HD inline
#endif

namespace ds2 {

// Tile sizes (the kernels' own constants; gemm.hip / bgemm.hip static_assert the match)
constexpr int kG16M = 128, kG16N = 128, kG16K = 16;   // sgemm_kernel (BM, BN, BK)
constexpr int kG64K = 64;                             // sgemm64_kernel (K64), 128 x 128/160
constexpr int kGB16K = 64;                            // sbgemm_kernel (KB16), 128 x 128
constexpr int kGX2M = 256, kGXS = 32;                 // sxgemm2_kernel (X2M, XS), 256 x 128/160
constexpr int kGBgM = 256, kGBgN = 256, kGBgK = 64;   // bgemm_nt_kernel (BG_M, BG_N, BG_K)

DS2_HD int gh_min(int a, int b) { return a < b ? a : b; }

// Work items (block id in dispatch order):
//   [0, main_wgs)       one whole output tile each (batch == 1), XCD-aware order;
//   [main_wgs, grid)    "tail" pieces: (batch, split, tile) of the tiles from tail_tile0
//                       on, K range split nsplit ways; dispatched last, they fill the
//                       slots the whole tiles leave in the final round.
// XCD-aware (bijective) remap of both ranges: the blocks the dispatcher deals to one XCD
// (ids congruent mod 8) get a contiguous run of tiles (pieces) in the grouped order below,
// so workgroups sharing an operand panel share that XCD's L2.
// Grouped tile order: tile ids run over groups of g_tile_group m-rows, inside a group column
// by column (m fastest), so the ~32 tiles one XCD runs at once span 4 m-rows x 8 n-columns
// (A: 4 panels, B: 8) instead of ~2 m-rows x every n-column (the input projection's 15 B
// panels, 7.7 MB, overflow the XCD's 4-MB L2 and were fetched again for every m-row).
// ds2_test_sgemm_cover enumerates these two functions on the host for a whole grid.
constexpr int kTileGroup = 4;

DS2_HD void tile_coords(int tile, int tn, int tm, int& tile_m, int& tile_n) {
  constexpr int G = kTileGroup;
  const int g = tile / (G * tn);
  const int rem = tile - g * G * tn;
  const int rows = gh_min(G, tm - g * G);
  tile_n = rem / rows;
  tile_m = g * G + (rem - tile_n * rows);
}

// bid, nblk: the kernels pass blockIdx.x, gridDim.x
DS2_HD void decode_work(int bid, int nblk, int M, int N, int K, int main_wgs, int tail_tile0,
                        int tail_tiles, int nsplit, int kchunk, float* partial, int& m0, int& n0,
                        int& kbeg, int& kend, int& bz, float*& part, int bn = kG16N,
                        int bm = kG16M) {
  const int tn = (N + bn - 1) / bn;
  const int orig = bid;
  int tile, z = 0;
  part = nullptr;
  if (orig < main_wgs) {
    const int q = main_wgs >> 3, r = main_wgs & 7;
    const int xcd = orig & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  } else {
    const int np = nblk - main_wgs;
    const int o = orig - main_wgs;
    const int q = np >> 3, r = np & 7;
    const int xcd = o & 7;
    const int pidx = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (o >> 3);
    z = pidx / tail_tiles;
    const int lt = pidx - z * tail_tiles;
    tile = tail_tile0 + lt;
    if (nsplit > 1) part = partial + ((int64_t)z * tail_tiles + lt) * (bm * bn);
  }
  int tile_m, tile_n;
  tile_coords(tile, tn, (M + bm - 1) / bm, tile_m, tile_n);
  // z = batch * nsplit + split
  bz = z / nsplit;
  const int sp = z - bz * nsplit;
  kbeg = orig < main_wgs ? 0 : sp * kchunk;
  kend = orig < main_wgs ? K : gh_min(K, kbeg + kchunk);
  m0 = tile_m * bm;
  n0 = tile_n * bn;
}

// bgemm.hip's decode: whole tiles first, then the split-K tail pieces (the same XCD-aware
// bijective remap as decode_work, grouped tile order of 4 tile rows; no batch).
DS2_HD void bg_decode(int bid, int nblk, int M, int N, int K, int main_wgs, int tail_tile0,
                      int tail_tiles, int nsplit, int kchunk, float* partial, int& m0, int& n0,
                      int& kbeg, int& kend, float*& part) {
  const int tn = (N + kGBgN - 1) / kGBgN, tm = (M + kGBgM - 1) / kGBgM;
  const int orig = bid;
  int tile, z = 0;
  part = nullptr;
  if (orig < main_wgs) {
    const int q = main_wgs >> 3, r = main_wgs & 7;
    const int xcd = orig & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  } else {
    const int np = nblk - main_wgs;
    const int o = orig - main_wgs;
    const int q = np >> 3, r = np & 7;
    const int xcd = o & 7;
    const int pidx = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (o >> 3);
    z = pidx / tail_tiles;
    const int lt = pidx - z * tail_tiles;
    tile = tail_tile0 + lt;
    if (nsplit > 1) part = partial + ((int64_t)z * tail_tiles + lt) * (kGBgM * kGBgN);
  }
  constexpr int G = 4;
  const int g = tile / (G * tn);
  const int rem = tile - g * G * tn;
  const int rows = gh_min(G, tm - g * G);
  const int tile_n = rem / rows;
  const int tile_m = g * G + (rem - tile_n * rows);
  kbeg = orig < main_wgs ? 0 : z * kchunk;
  kend = orig < main_wgs ? K : gh_min(K, kbeg + kchunk);
  m0 = tile_m * kGBgM;
  n0 = tile_n * kGBgN;
}

// ---------------------------------------------------------------------------------------------
// Host only from here on.

inline int gh_cdiv(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }

// Work plan.  Whole tiles run in full rounds of `slots` resident workgroups; the tiles of a
// last, partial round ("tail") have their K range split so that the round is filled.  On 256
// CUs: 16032 x 2400 on the BK=16 kernel's 128-wide tiles (3 workgroups per CU) = 2394 tiles
// = 3 rounds of 768 + 90 tail tiles x 8 splits (K = 2048, 256-k pieces); the weight gradient
// 2400 x 800 (K = 16032) on the fp16x3 kernel's 256 x 160 tiles = 50 tiles x 5 splits of
// 3232 k.  Split partials are reduced in a fixed order.
struct GemmPlan {
  int main_wgs, tail_tile0, tail_tiles, nsplit, kchunk, bn, bm;
};

// Plan for tile width bn.  The split count s of the tail is chosen by a time model in
// units of one workgroup slot's MFMA time per (128-row x k) tile step: whole rounds
// cost k each, the tail ceil(pieces / slots) * kchunk; a split adds its partial-slab
// write + read (8 B per element at ~4 TB/s) and the reduce launch.  `eff` is the tile's
// relative MFMA efficiency (160-wide tiles: 5 B fragments per 4 A, measured ~7 % faster
// per unit of work than 128-wide in isolation; 1.15 in the plan, where it also stands in
// for the 160-wide tile's smaller tail: a whole training step measured 1.0 < 1.07 < 1.15
// ~ 1.25 ~ 1.4, the last three within noise).
struct PlanChoice {
  GemmPlan p;
  double t;   // seconds (model)
};

inline PlanChoice plan_bn(int m, int n, int k, int batch, int bn, int slots, int bk, double eff,
                          int bm = kG16M) {
  const int tiles = gh_cdiv(m, bm) * gh_cdiv(n, bn);
  GemmPlan p{0, 0, tiles, 1, std::max(k, 1), bn, bm};
  if (batch == 1) {
    p.main_wgs = (tiles / slots) * slots;
    p.tail_tile0 = p.main_wgs;
    p.tail_tiles = tiles - p.main_wgs;
    if (p.tail_tiles == 0) {   // full rounds only
      p.main_wgs = 0;
      p.tail_tile0 = 0;
      p.tail_tiles = tiles;
    }
  }
  // seconds per unit (one k step of one BM x bn tile on one slot)
  const double unit = 2.0 * bm * bn / (157.3e12 * eff / slots);
  const double main_t = (double)(p.main_wgs / slots) * k * unit;
  const int64_t tail = (int64_t)p.tail_tiles * batch;
  const int smax = std::max(1, std::min(32, k / 256));
  double best = 1e30;
  int bs = 1;
  for (int s = 1; s <= smax; ++s) {
    const int kc = gh_cdiv(gh_cdiv(k, s), bk) * bk;
    const int ns = gh_cdiv(k, kc);
    if (s > 1 && ns != s) continue;
    const int64_t pieces = tail * ns;
    double t = (double)((pieces + slots - 1) / slots) * kc * unit;
    if (ns > 1) t += (double)pieces * bm * bn * 8.0 / 4e12 + 6e-6;
    if (t < best - 1e-12) {
      best = t;
      bs = ns;
    }
  }
  if (bs > 1) {
    p.kchunk = gh_cdiv(gh_cdiv(k, bs), bk) * bk;
    p.nsplit = gh_cdiv(k, p.kchunk);
  }
  return {p, main_t + best};
}

// 160-wide tiles are ~7 % faster per unit of work than 128-wide in isolation (5 B fragments
// per 4 A); 1.15 in the time model, where it also stands in for the 160-wide tile's smaller
// tail (a whole training step measured 1.0 < 1.07 < 1.15 ~ 1.25 ~ 1.4, the last three
// within noise)
constexpr double kEff160 = 1.15;

// the fp32-MFMA kernels: BK=16 (3 workgroups per CU) or, k64, the deep-K one (2 per CU)
inline GemmPlan gemm_plan(int m, int n, int k, int batch, bool k64, int cus) {
  if (!k64) return plan_bn(m, n, k, batch, kG16N, 3 * cus, kG16K, 1.0).p;
  const PlanChoice a = plan_bn(m, n, k, batch, 128, 2 * cus, kG64K, 1.0);
  const PlanChoice b = plan_bn(m, n, k, batch, 160, 2 * cus, kG64K, kEff160);
  return b.t < a.t ? b.p : a.p;
}

inline size_t plan_ws(const GemmPlan& p, int batch) {
  return p.nsplit > 1 ? (size_t)p.nsplit * batch * p.tail_tiles * p.bm * p.bn * sizeof(float) + 256
                      : 0;
}

// the bf16x6 kernel: 256-row tiles, one workgroup per CU, split-K in 32-k chunks; 160-wide
// tiles measured faster on every step shape with N >= 800 (scripts/bench_gemm_x6.py: 180-201
// vs 159-194 TF), 128-wide on narrow N (the FC's 29 columns)
inline GemmPlan x6_plan(int m, int n, int k, int batch, int cus) {
  return plan_bn(m, n, k, batch, n >= 256 ? 160 : 128, cus, kGXS, 1.0, kGX2M).p;
}

// the staged-bf16 kernel (sbgemm_kernel): 128 x 128 tiles, 2 workgroups per CU
inline GemmPlan bf16_plan(int m, int n, int k, int batch, int cus) {
  return plan_bn(m, n, k, batch, 128, 2 * cus, kGB16K, 1.0).p;
}

// fp16x3 row-scale words after the split-K slabs
inline size_t h3_ws(int m, int n) { return (size_t)(m + n) * 4 + 512; }

// bgemm_nt_kernel: whole tiles in full rounds of one workgroup per CU; the last partial
// round's tiles get their K range split so the pieces fill a round (time model in units of one
// 64-deep tile step; a split piece adds its 256 KB partial slab written and read back, ~1/8 of
// a step).
inline GemmPlan bg_plan(int m, int n, int k, int cus) {
  const int tiles = gh_cdiv(m, kGBgM) * gh_cdiv(n, kGBgN);
  GemmPlan p{(tiles / cus) * cus, 0, 0, 1, k, kGBgN, kGBgM};
  p.tail_tile0 = p.main_wgs;
  p.tail_tiles = tiles - p.main_wgs;
  if (p.tail_tiles == 0) {
    p.main_wgs = 0;
    p.tail_tile0 = 0;
    p.tail_tiles = tiles;
  }
  const int ksteps = gh_cdiv(k, kGBgK);
  double best = 1e30;
  for (int s = 1; s <= 32 && s <= ksteps; ++s) {
    const int kc = gh_cdiv(ksteps, s);
    const int ns = gh_cdiv(ksteps, kc);
    if (s > 1 && ns != s) continue;
    const int64_t pieces = (int64_t)p.tail_tiles * ns;
    const double t = (double)((pieces + cus - 1) / cus) * kc +
                     (ns > 1 ? 0.125 * (double)pieces / cus + 1.0 : 0.0);
    if (t < best - 1e-9) {
      best = t;
      p.nsplit = ns;
      p.kchunk = kc * kGBgK;
    }
  }
  if (p.nsplit == 1) p.kchunk = k;
  return p;
}

// The environment switches.  DS2_GEMM_X6=0 selects the fp32-MFMA kernels (the accuracy
// cross-check of the tests); DS2_GEMM_H3=0 the bf16x6 kernel where fp16x3 would run.
struct GemmSwitches {
  bool x6, h3;
};
inline GemmSwitches gemm_switches() {
  const char* x = getenv("DS2_GEMM_X6");
  const char* h = getenv("DS2_GEMM_H3");
  return {!(x != nullptr && x[0] == '0'), !(h != nullptr && h[0] == '0')};
}

// What a call is: the scalar arguments and the addresses (only their low bits and whether
// they are null are used).  kind 0: ds2_sgemm / ds2_sgemm_ws / ds2_sgemm_amax_ws, 1:
// ds2_sgemm_bf16_ws, 2: ds2_bgemm_nt (trans_a 0, trans_b 1, batch 1, strides 0; ld in bf16).
struct GemmCall {
  int kind, trans_a, trans_b, m, n, k;
  uintptr_t a;
  int64_t lda, stride_a;
  uintptr_t b;
  int64_t ldb, stride_b;
  uintptr_t c;
  int64_t ldc, stride_c;
  int batch;
  uintptr_t bias;
  bool have_ws;
  size_t ws_bytes;
};

struct GemmChoice {
  ds2_status_t status;   // what the entry point returns before any launch (OK: go on)
  int rung;              // DS2_GEMM_*; NONE with status OK: nothing to do (an empty product)
  GemmPlan p;
  int64_t grid;          // workgroups of the GEMM kernel
  bool va, vb;           // float4 staging of A / B is legal (BK=16 kernel's template flags)
  bool fits;             // both operands span < 2^31 bytes (32-bit buffer offsets)
  bool kalign;           // every stage of every piece lies wholly inside [0, K)
  bool m16, h3;          // 16x16x32 form; fp16x3
  bool vec;              // 16-B form of the split reduce / of bgemm's C rows (cvec)
  size_t slabs;          // split-K slab bytes (0 without a split)
  size_t ws_need;        // workspace bytes the rung uses: slabs, + the fp16x3 scale words
};

inline bool gh_aligned16(uintptr_t p) { return (p & 15) == 0; }

// 32-bit buffer offsets: each operand (one batch entry) must span < 2^31 bytes
inline bool fits_rsrc(int64_t rows, int64_t ld) { return rows * ld * 4 < (1ll << 31); }

// The one selection.  K = 0 is rejected (DS2_UNSUPPORTED_SHAPE): the split-operand kernels
// issue their first stage's loads before they test the K range.
inline GemmChoice gemm_select(const GemmCall& g, const GemmSwitches& sw, int cus) {
  GemmChoice ch{};
  ch.status = DS2_OK;
  ch.rung = DS2_GEMM_NONE;
  const int m = g.m, n = g.n, k = g.k, batch = g.batch;
  if (g.kind == 2) {
    if (m < 0 || n < 0 || k < 0) return ch.status = DS2_INVALID_VALUE, ch;
    if (m == 0 || n == 0) return ch;
    if (g.a == 0 || g.b == 0 || g.c == 0 || g.lda < k || g.ldb < k || g.ldc < n)
      return ch.status = DS2_INVALID_VALUE, ch;
    // 16-B DMA granules: 16-B aligned operands, k and the row strides multiples of 8 bf16
    if ((g.a & 15) || (g.b & 15) || (g.lda & 7) || (g.ldb & 7) || (k & 7) ||
        (int64_t)m * g.lda * 2 >= (1ll << 31) || (int64_t)n * g.ldb * 2 >= (1ll << 31) ||
        g.lda >= (1 << 30) || g.ldb >= (1 << 30))
      return ch.status = DS2_UNSUPPORTED_SHAPE, ch;
    if (k == 0) return ch.status = DS2_UNSUPPORTED_SHAPE, ch;
    ch.va = ch.vb = ch.fits = true;
    ch.p = bg_plan(m, n, k, cus);
    if (ch.p.nsplit > 1 && (!g.have_ws || g.ws_bytes < plan_ws(ch.p, 1))) {
      ch.p.nsplit = 1;
      ch.p.kchunk = k;
    }
    ch.grid = ch.p.main_wgs + (int64_t)ch.p.tail_tiles * ch.p.nsplit;
    if (ch.grid > 0x7fffffff) return ch.status = DS2_UNSUPPORTED_SHAPE, ch;
    ch.kalign = k % kGBgK == 0 && ch.p.kchunk % kGBgK == 0;
    // 16-B row runs of C (and of bias) when every row starts 16-B aligned
    ch.vec = !((g.c & 15) || (g.ldc & 3) || (g.bias != 0 && (g.bias & 15)));
    ch.slabs = ch.ws_need = plan_ws(ch.p, 1);
    ch.rung = ch.kalign ? DS2_GEMM_BF16_DMA : DS2_GEMM_BF16_DMA_K;
    return ch;
  }
  if (m < 0 || n < 0 || k < 0 || batch < 0) return ch.status = DS2_INVALID_VALUE, ch;
  if (m == 0 || n == 0 || batch == 0) return ch;
  if (g.ldc < n) return ch.status = DS2_INVALID_VALUE, ch;
  if (g.trans_a ? g.lda < m : g.lda < k) return ch.status = DS2_INVALID_VALUE, ch;
  if (g.trans_b ? g.ldb < k : g.ldb < n) return ch.status = DS2_INVALID_VALUE, ch;
  if (k == 0) return ch.status = DS2_UNSUPPORTED_SHAPE, ch;
  // vector (float4) staging is legal when every float4 is fully in or out of bounds
  ch.va = gh_aligned16(g.a) && (g.lda % 4 == 0) && (g.stride_a % 4 == 0) &&
          (g.trans_a ? (m % 4 == 0) : (k % 4 == 0));
  ch.vb = gh_aligned16(g.b) && (g.ldb % 4 == 0) && (g.stride_b % 4 == 0) &&
          (g.trans_b ? (k % 4 == 0) : (n % 4 == 0));
  ch.fits = fits_rsrc(g.trans_a ? k : m, g.lda) && fits_rsrc(g.trans_b ? n : k, g.ldb);
  bool x6 = false, k64 = false;
  if (g.kind == 1) {
    // every operand must be float4-staged and span < 2^31 bytes (no silent fp32 fallback)
    if (!ch.va || !ch.vb || !ch.fits) return ch.status = DS2_UNSUPPORTED_SHAPE, ch;
    ch.p = bf16_plan(m, n, k, batch, cus);
  } else {
    // the bf16x6 / fp16x3 kernel needs float4-staged operands; the fp32 kernels take any
    // alignment: the deep-K one for float4-staged operands, BK=16 for the rest
    x6 = ch.fits && ch.va && ch.vb && sw.x6;
    k64 = !x6 && ch.va && ch.vb && ch.fits;
    ch.p = x6 ? x6_plan(m, n, k, batch, cus) : gemm_plan(m, n, k, batch, k64, cus);
  }
  // The workspace ladder: one that cannot hold the plan's split-K slabs is not used at all
  // (whole-K pieces, no fp16x3 scale words in it either); with the slabs but no room for the
  // scale words after them the split runs on the bf16x6 kernel; with both, fp16x3.
  bool use_ws = g.have_ws;
  if (ch.p.nsplit > 1 && (!g.have_ws || g.ws_bytes < plan_ws(ch.p, batch))) {
    ch.p.nsplit = 1;                       // no workspace: whole-K pieces
    ch.p.kchunk = std::max(k, 1);
    use_ws = false;
  }
  ch.grid = ch.p.main_wgs + (int64_t)ch.p.tail_tiles * batch * ch.p.nsplit;
  if (ch.grid > 0x7fffffff) return ch.status = DS2_UNSUPPORTED_SHAPE, ch;
  ch.slabs = ch.p.nsplit > 1 ? plan_ws(ch.p, batch) : 0;
  ch.ws_need = ch.slabs;
  if (g.kind == 1) {
    ch.kalign = false;                     // sbgemm_kernel checks k per stage
    ch.vec = false;                        // and its reduce is the scalar form
    ch.rung = DS2_GEMM_BF16_STAGED;
    return ch;
  }
  ch.kalign = k % kGXS == 0 && (ch.p.nsplit == 1 || ch.p.kchunk % kGXS == 0);
  // the 16x16x32 form wherever every stage lies inside K (r4d: 0-15 % faster on the step's
  // shapes, profiles/r4d_gemm_x6_m16_sk_ab.txt), the 32x32x16 form for a K tail
  ch.m16 = x6 && ch.kalign;
  ch.h3 = ch.m16 && batch == 1 && sw.h3 && use_ws && g.ws_bytes >= ch.slabs + h3_ws(m, n);
  if (ch.h3) ch.ws_need = ch.slabs + h3_ws(m, n);
  ch.vec = ch.p.nsplit > 1 && ch.p.bn % 4 == 0 && gh_aligned16(g.c) && g.ldc % 4 == 0 &&
           g.stride_c % 4 == 0 && (g.bias == 0 || gh_aligned16(g.bias));
  const bool w = ch.p.bn == 160;
  if (ch.h3) ch.rung = w ? DS2_GEMM_H3_160 : DS2_GEMM_H3_128;
  else if (ch.m16) ch.rung = w ? DS2_GEMM_X6_M16_160 : DS2_GEMM_X6_M16_128;
  else if (x6) ch.rung = w ? DS2_GEMM_X6_K_160 : DS2_GEMM_X6_K_128;
  else if (k64) ch.rung = w ? DS2_GEMM_F64_160 : DS2_GEMM_F64_128;
  else ch.rung = DS2_GEMM_F16;
  return ch;
}

// The workspace the size queries promise: enough for any rung the call can land on, whatever
// the operand alignment and the switches.
inline size_t gemm_ws_any(int m, int n, int k, int batch, int cus) {
  return std::max(std::max(plan_ws(gemm_plan(m, n, k, batch, false, cus), batch),
                           plan_ws(gemm_plan(m, n, k, batch, true, cus), batch)),
                  plan_ws(x6_plan(m, n, k, batch, cus), batch) + h3_ws(m, n));
}

// ds2_test_sgemm_cover: every workgroup id of the grid through the kernels' own decode.
// Returns the (batch, tile) pairs whose pieces do not partition [0, K) exactly once plus the
// decoded tiles outside the tile grid; -1 for arguments no plan has.
// 256 x 256 tiles are bgemm's (bg_decode, batch 1); every other tile goes through decode_work.
inline int64_t gemm_cover_defects(int m, int n, int k, int batch, int bm, int bn, int main_wgs,
                                  int tail_tile0, int tail_tiles, int nsplit, int kchunk,
                                  int grid) {
  if (m < 1 || n < 1 || k < 1 || batch < 1 || bm < 1 || bn < 1 || main_wgs < 0 ||
      tail_tile0 < 0 || tail_tiles < 1 || nsplit < 1 || kchunk < 1 || grid < main_wgs)
    return -1;
  const bool bg = bm == kGBgM && bn == kGBgN;
  if (bg && batch != 1) return -1;
  const int tm = gh_cdiv(m, bm), tn = gh_cdiv(n, bn);
  const int64_t pairs = (int64_t)batch * tm * tn;
  struct Piece {
    int64_t pair;
    int kbeg, kend;
  };
  std::vector<Piece> pieces;
  pieces.reserve(grid);
  int64_t outside = 0;
  for (int bid = 0; bid < grid; ++bid) {
    int m0, n0, kbeg, kend, bz = 0;
    float* part;
    if (bg)
      bg_decode(bid, grid, m, n, k, main_wgs, tail_tile0, tail_tiles, nsplit, kchunk, nullptr, m0,
                n0, kbeg, kend, part);
    else
      decode_work(bid, grid, m, n, k, main_wgs, tail_tile0, tail_tiles, nsplit, kchunk, nullptr,
                  m0, n0, kbeg, kend, bz, part, bn, bm);
    if (m0 < 0 || n0 < 0 || m0 % bm != 0 || n0 % bn != 0 || m0 / bm >= tm || n0 / bn >= tn ||
        bz < 0 || bz >= batch) {
      ++outside;
      continue;
    }
    pieces.push_back({((int64_t)bz * tm + m0 / bm) * tn + n0 / bn, kbeg, kend});
  }
  // bucket the pieces by pair (counting sort), then walk each pair's pieces in k order
  std::vector<int64_t> first(pairs + 1, 0);
  for (const Piece& p : pieces) ++first[p.pair + 1];
  for (int64_t i = 0; i < pairs; ++i) first[i + 1] += first[i];
  std::vector<Piece> by(pieces.size());
  {
    std::vector<int64_t> at(first.begin(), first.end() - 1);
    for (const Piece& p : pieces) by[at[p.pair]++] = p;
  }
  int64_t bad = 0;
  for (int64_t i = 0; i < pairs; ++i) {
    Piece* b = by.data() + first[i];
    Piece* e = by.data() + first[i + 1];
    std::sort(b, e, [](const Piece& x, const Piece& y) { return x.kbeg < y.kbeg; });
    int at = 0;
    bool ok = true;
    for (Piece* p = b; p != e; ++p) {
      if (p->kbeg != at || p->kend <= p->kbeg) ok = false;
      at = p->kend;
    }
    if (!ok || at != k) ++bad;
  }
  return bad + outside;
}

}  // namespace ds2
