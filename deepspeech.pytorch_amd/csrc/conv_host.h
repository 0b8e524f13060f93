// Host side of the Conv2d dispatch (conv.hip, conv_split.hip): the shape, the geometry host and
// device share, the tile limits the predicates test, the environment switches, and one plan
// per direction -- which kernel runs (the rung), the workspace it needs with every offset
// into it, and the grid numbers the host computes.  The entry points, the two workspace
// queries and ds2_test_conv2d_plan all go through conv_plan_*; nothing else decides.
// DESIGN.md "Conv2d dispatch" has the ladder per direction; INTEGRATION.md the switches.
#pragma once

#include "split_mma.h"

#include <algorithm>
#include <cstdlib>

namespace ds2 {

struct ConvDims {
  int n, ci, hi, wi, co, kh, kw, sh, sw, ph, pw, ho, wo;
};

static inline bool make_dims(ConvDims& g, int n, int c_in, int h_in, int w_in, int c_out, int kh,
                             int kw, int sh, int sw, int ph, int pw) {
  if (n < 0 || c_in < 1 || h_in < 1 || w_in < 1 || c_out < 1 || kh < 1 || kw < 1 || sh < 1 ||
      sw < 1 || ph < 0 || pw < 0)
    return false;
  // a kernel larger than the padded input: the division below truncates toward zero and would
  // give one output row / column for a deficit smaller than the stride
  if (h_in + 2 * ph < kh || w_in + 2 * pw < kw) return false;
  g = ConvDims{n, c_in, h_in, w_in, c_out, kh, kw, sh, sw, ph, pw, 0, 0};
  g.ho = (h_in + 2 * ph - kh) / sh + 1;
  g.wo = (w_in + 2 * pw - kw) / sw + 1;
  return g.ho >= 1 && g.wo >= 1;
}

// --- tile limits (the kernels' comments say what each one is) -------------------------------
// fp32 LDS-patch forward / dgrad (conv_patch_kernel)
constexpr int PT_ROWS = 4;          // output rows per workgroup (one per wave)
constexpr int PT_COLS = 128;        // output columns per workgroup
constexpr int PT_PITCH = 144;       // patch row pitch (>= PT_COLS + kw - 1)
constexpr int PT_PROWS = 28;        // max patch rows incl. one zero row
constexpr int PT_TMAX = 232;        // max taps (padded to even)
constexpr int PT_WP = 33;           // tap-row pitch of the weight tile (conflict-free)
// fp32 LDS-tile weight gradient (conv_wgrad_patch_kernel)
constexpr int WG_RW = 2;            // output rows per chunk
constexpr int WG_CW = 128;          // output columns per chunk
constexpr int WG_XS_SMALL = 3200;   // x patch floats, <= 8 tap tiles (conv2: 23 x 139)
constexpr int WG_XS_LARGE = 11520;  // x patch floats, <= 16 tap tiles (conv1: 43 x 267)
// single-channel patch forward (conv1_patch_fwd_kernel)
constexpr int C1_RW = 4;
constexpr int C1_WC = 128;
constexpr int C1_T = 512;
constexpr int C1_PATCH = 12560;     // floats: ((C1_RW - 1) sh + kh) x ((C1_WC - 1) sw + kw2)
constexpr int C1_KROWS = 492;       // filter-bank rows kh x kw2 (conv1: 41 x 12)
// bf16x6 / fp16x3 forward and dgrad (conv_x6_kernel and the two-row kernels)
constexpr int CX_T = 512;
constexpr int CX_COLS = 256;
constexpr int CX_PATCH = 3 * 522 * 24;   // bf16: 3 planes x columns x pitch (max)
constexpr int CX_PATCH1 = 3 * 267 * 40;  // the same for width stride 1 without row chunks
constexpr int CX_PATCH_DB = 2 * 3 * 267 * 24;   // double-buffered (conv2 fwd: pitch 24)
constexpr int CX_WIMG = 3 * 32 * 296;    // bf16: 3 planes x 32 channels x COP (max)
constexpr int CX_PU = 3;                 // patch staging units per thread (max; template PU)
constexpr int CX_WQ = 7;                 // 16-B weight-image chunks per thread
// 4 x 2-fragment dgrad (conv_x6q_dgrad_kernel, conv_h3_dgrad2r_kernel)
constexpr int CQ_ROWS = 12;              // class tap rows, padded to 4
constexpr int CQ_COP = 152;              // weight-image ci pitch: 8 x odd >= 144
// bf16x6 / fp16x3 weight gradients (conv_x6_wgrad_kernel, conv_x6_wgrad_sw_kernel)
constexpr int CW_T = 256;
constexpr int CW_SLOTS = 512;              // workgroups per launch (two per CU)
constexpr int X6W_BLOCK = 32 * 4 * 32;     // floats per (co, w, ci) plane of one kernel column
constexpr int SW_COLS = 32;                // output columns per row stage (two 16-column k-steps)

// --- geometry shared by host and device -----------------------------------------------------
__host__ __device__ inline int class_taps(const ConvDims& g, int q) {
  return q < g.kh ? (g.kh - 1 - q) / g.sh + 1 : 0;
}

// dgrad, stride class q (input rows hi with (hi + ph) % sh == q): its first row *hq and how
// many rows it has
__host__ __device__ inline int class_rows(const ConvDims& g, int q, int* hq) {
  *hq = ((q - g.ph) % g.sh + g.sh) % g.sh;
  return *hq < g.hi ? (g.hi - 1 - *hq) / g.sh + 1 : 0;
}

// weight-image geometry of the fp32 patch kernels: tap rows padded to even, 33-float rows,
// tiles padded to 16 bytes
__host__ __device__ inline int wimg_tstride(const ConvDims& g, bool dgrad) {
  const int a = dgrad ? class_taps(g, 0) : g.kh;   // class 0 has the most taps
  return ((a * g.kw) + 1) & ~1;
}
__host__ __device__ inline int64_t wimg_tile(int tstride) {
  return ((int64_t)tstride * PT_WP + 3) & ~(int64_t)3;
}

struct CxGeom {
  int KA;     // tap rows (of one chunk) padded to 8
  int NBP;    // kernel-column pairs
  int P;      // patch column pitch (bf16)
  int COP;    // weight-image channel pitch (bf16)
  int PCOL;   // patch columns
  int RC;     // tap-row chunks per loop channel
};

__host__ __device__ constexpr int cx_pitch8odd(int v) {   // smallest 8 * odd >= v
  return 8 * (((v + 7) / 8) % 2 == 0 ? (v + 7) / 8 + 1 : (v + 7) / 8);
}

// The geometry cx_geom gives an instantiation with compile-time a-groups / column pairs and
// width stride 1 without row chunks (conv2 fwd / dgrad): with it a compile-time constant,
// every fragment read is one per-lane base + an immediate offset (no address registers or
// VALU per k-step).
template <int NGA, int NBP>
struct CxConst {
  static constexpr int KA = 8 * NGA;
  static constexpr int P = cx_pitch8odd(KA);
  static constexpr int COP = cx_pitch8odd(2 * NBP * KA + 1);
  static constexpr int PCOL = (256 - 1) + 2 * NBP;
};

__host__ __device__ inline CxGeom cx_geom(const ConvDims& g, bool dgrad) {
  CxGeom c;
  const int a = dgrad ? class_taps(g, 0) : g.kh;
  c.KA = a <= 24 ? (a + 7) / 8 * 8 : 16;
  c.RC = (a + c.KA - 1) / c.KA;
  c.NBP = (g.kw + 1) / 2;
  c.P = cx_pitch8odd(c.KA);        // 8 x odd bf16: conflict-free 16-B fragment reads
  c.COP = cx_pitch8odd(2 * c.NBP * c.KA + 1);
  c.PCOL = (CX_COLS - 1) * (dgrad ? 1 : g.sw) + 2 * c.NBP;
  return c;
}
// the compile-time-geometry instantiations must see the geometry cx_geom computed
template <int NGA>
static inline bool cx_is_const6(const CxGeom& c) {
  typedef CxConst<NGA, 6> K;
  return c.KA == K::KA && c.P == K::P && c.COP == K::COP && c.PCOL == K::PCOL && c.NBP == 6;
}

// --- device helpers both files' kernels use ---------------------------------------------------
// XCD-aware decode of a 3-D grid launched as gx*gy*gz 1-D blocks: the blocks one XCD
// is dealt (ids congruent mod 8) get a contiguous run of (x fastest, y, z) tiles, so
// tiles that share input rows / samples share that XCD's L2.  Speed only.
__device__ __forceinline__ void xcd_tile(int gx, int gy, int& bx, int& by, int& bz) {
  const int nwg = gridDim.x;
  const int o = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = o & 7;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (o >> 3);
  bx = id % gx;
  by = (id / gx) % gy;
  bz = id / (gx * gy);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_rsrc(const float* p, int64_t elems) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), (short)0,
                                           static_cast<int>(elems * 4), 0x00020000);
}

// --- environment switches: read once per call, never cached (the tests flip them) -----------
struct ConvSwitches {
  bool x6;         // DS2_CONV_X6: the bf16x6 / fp16x3 kernels (0: the fp32 kernels)
  bool h3;         // DS2_CONV_H3: fp16x3 for the conv2-shaped forward and the 4 x 2 dgrad
  bool two_row;    // DS2_CONV_2R: two output rows per workgroup in those fp16x3 kernels
  bool h3w;        // DS2_CONV_H3W: fp16x3 for the sliding-window weight gradient
  bool w64;        // DS2_CONV_W64: that weight gradient on 64-column row stages (opt-in)
  bool dg_flush;   // DS2_CONV_DG_FLUSH: the one-row fp16x3 dgrad's per-channel chain flush
};
static inline ConvSwitches conv_switches() {
  // on unless the variable starts with '0'; W64 is opt-in ('1'); DG_FLUSH is off at any zero
  const auto env = [](const char* name) { return getenv(name); };
  const auto on = [&](const char* name) { return !(env(name) != nullptr && env(name)[0] == '0'); };
  const char *w = env("DS2_CONV_W64"), *f = env("DS2_CONV_DG_FLUSH");
  return ConvSwitches{on("DS2_CONV_X6"), on("DS2_CONV_H3"), on("DS2_CONV_2R"), on("DS2_CONV_H3W"),
                      w != nullptr && w[0] == '1', !(f != nullptr && atoi(f) == 0)};
}

// --- plans ------------------------------------------------------------------------------------
// The rungs are the DS2_CONV_* values of include/ds2hip_test.h, one per kernel instantiation
// (conv1_patch_fwd_kernel<KWH> and conv_wgrad_patch_kernel<NT, XS, SW> as families with
// their parameters in a / b).
struct ConvPlan {
  int rung = DS2_CONV_NONE;
  int a = 0, b = 0;          // FWD_C1: KWH, 0; WG_PATCH: NT, SW; the x6 wgrads: tap rows per
                             // group (nw), groups (G)
  size_t ws_bytes = 0;       // what the rung needs of the caller's workspace
  // byte offsets into the workspace; the weight image / the partial slabs start at 0
  size_t m_exp = 0, n_amax = 0;      // fp16x3 scales of forward and dgrad
  size_t co_amax = 0, ci_amax = 0;   // fp16x3 channel maxima of the weight gradient
  int64_t img = 0;           // elements of one weight-image plane (fp32 patch: of the image)
  int gx = 0;                // column tiles
  int gy = 0;                // rows / row pairs / row tiles per (sample, channel block)
  int64_t grid = 0;          // workgroups of the convolution kernel
  bool too_big = false;      // the one-row grid of the shape exceeds 2^31 - 1 workgroups
  bool h3 = false;           // an fp16x3 rung: the scales / channel maxima are computed first
  int splits = 0, bands = 0, pitch = 0;   // wgrad: partial slabs = splits (x6) or n * bands
  int tstride = 0;           // fp32 patch fwd / dgrad: taps per weight tile
};

static inline size_t conv_align256(size_t b) { return (b + 255) / 256 * 256; }
// gx * gy tiles for each of `per` (sample, channel block) pairs
static inline void plan_grid(ConvPlan& p, int64_t per) {
  p.grid = (int64_t)p.gx * p.gy * per;
  p.too_big = p.too_big || p.grid > 0x7fffffff;
}
static inline bool fits_buf32(int64_t elems) { return elems * 4 < (1ll << 31) - 64; }

// split-weight image of `elems` values per plane: 3 bf16 planes, or 2 fp16 planes + the
// fp16x3 scales (m_exp[M] int, n_amax[n] unsigned) at the next 256-B boundary; the workspace
// covers either, whichever H3 says
static inline void plan_cx_ws(ConvPlan& p, int64_t elems, int M, int n) {
  p.img = elems;
  p.m_exp = conv_align256((size_t)elems * 2 * sizeof(unsigned short));
  p.n_amax = p.m_exp + (size_t)M * 4;
  p.ws_bytes = std::max((size_t)elems * 3 * sizeof(unsigned short), p.n_amax + (size_t)n * 4);
}

// Each family below fills `p` and returns whether it takes the shape.  A direction's plan is
// the first family that does; the fwd / dgrad workspace query is the largest ws_bytes over
// all that do (so a workspace sized once serves every switch setting of H3 / 2R / DG_FLUSH).

// bf16x6 / fp16x3 one-row family (conv_x6_kernel, conv_h3_fwd2r_kernel): width stride 1,
// <= 12 kernel columns, <= 24 tap rows (one chunk), patches and weight chunks that fit the
// LDS, planes within 32-bit buffer offsets.  conv1 (stride 2, 41 tap rows) stays on the fp32
// kernels: a bf16x6 form of it moved hardtanh inputs of the tiny golden batch across the kink
// (DESIGN.md §4).
static inline bool plan_x6(const ConvDims& g, const ConvSwitches& s, bool dgrad, ConvPlan& p) {
  if (!s.x6 || g.sw != 1 || g.kw < 1 || g.kw > 12) return false;
  const CxGeom c = cx_geom(g, dgrad);
  if (c.RC > 1) return false;
  if (c.KA > 24 || 3 * c.PCOL * c.P > CX_PATCH || 3 * 32 * c.COP > CX_WIMG) return false;
  if (c.PCOL * (c.KA / 8) > CX_PU * CX_T || 3 * 32 * c.COP / 8 > CX_WQ * CX_T) return false;
  if (!fits_buf32(dgrad ? (int64_t)g.ho * g.wo : (int64_t)g.hi * g.wi)) return false;
  const int M = dgrad ? g.ci : g.co, L = dgrad ? g.co : g.ci;
  const int mb = (M + 31) / 32;
  p = ConvPlan{};
  plan_cx_ws(p, (int64_t)(dgrad ? g.sh : 1) * mb * L * c.RC * 32 * c.COP, M, g.n);
  p.gx = cdiv(dgrad ? g.wi : g.wo, CX_COLS);
  p.gy = dgrad ? g.hi : g.ho;
  plan_grid(p, (int64_t)g.n * mb);
  // the compile-time instantiations: conv2's forward (3 tap-row groups x 6 column pairs,
  // double-buffered patch) and the 8-row-fragment dgrad (2 x 6)
  const bool fits1 = 3 * c.PCOL * c.P <= CX_PATCH1 && c.PCOL * (c.KA / 8) <= 2 * CX_T;
  if (dgrad) {
    p.rung = fits1 && cx_is_const6<2>(c) ? DS2_CONV_DG_X6_26 : DS2_CONV_DG_X6;
  } else if (fits1 && cx_is_const6<3>(c) && 2 * 3 * c.PCOL * c.P <= CX_PATCH_DB) {
    p.rung = !s.h3 ? DS2_CONV_FWD_X6_DB : g.sh == 2 && s.two_row ? DS2_CONV_FWD_H3_2R
                                                                 : DS2_CONV_FWD_H3_1R;
    p.h3 = s.h3;
    if (p.rung == DS2_CONV_FWD_H3_2R) {   // output rows r, r + 4 of every 8
      p.gy = 4 * (g.ho / 8) + std::min(4, g.ho % 8);
      plan_grid(p, (int64_t)g.n * mb);
    }
  } else {
    p.rung = DS2_CONV_FWD_X6;
  }
  return true;
}

// the 4 x 2-fragment dgrad (conv_x6q_dgrad_kernel, conv_h3_dgrad2r_kernel): width stride 1,
// <= 12 class tap rows and <= 12 kernel columns
static inline bool plan_x6q(const ConvDims& g, const ConvSwitches& s, ConvPlan& p) {
  if (!s.x6 || g.sw != 1 || g.kw < 1 || g.kw > 12 || class_taps(g, 0) > CQ_ROWS) return false;
  if (!fits_buf32((int64_t)g.ho * g.wo) || (int64_t)g.co * 3 * 32 * CQ_COP * 2 >= (1ll << 31) - 64)
    return false;
  const int mb = (g.ci + 31) / 32;
  p = ConvPlan{};
  plan_cx_ws(p, (int64_t)g.sh * mb * g.co * 32 * CQ_COP, g.ci, g.n);
  p.gx = cdiv(g.wi, CX_COLS);
  p.gy = g.hi;
  plan_grid(p, (int64_t)g.n * mb);
  p.h3 = s.h3;
  p.rung = !s.h3 ? DS2_CONV_DG_X6_Q : s.two_row ? DS2_CONV_DG_H3_2R
                 : s.dg_flush ? DS2_CONV_DG_H3_Q : DS2_CONV_DG_H3_Q_NOFLUSH;
  if (p.rung == DS2_CONV_DG_H3_2R) {   // per stride class: rows t, t + 4 of every 8
    p.gy = 0;
    for (int q = 0, hq; q < g.sh; ++q) {
      const int cnt = class_rows(g, q, &hq);
      p.gy += 4 * (cnt / 8) + std::min(4, cnt % 8);
    }
    plan_grid(p, (int64_t)g.n * mb);
  }
  return true;
}

// the fp32 LDS-patch kernel (conv_patch_kernel): width stride 1 with patches / tap tiles
// that fit its LDS
static inline bool plan_patch(const ConvDims& g, bool dgrad, ConvPlan& p) {
  if (g.sw != 1 || g.kw < 2 || g.kw > PT_PITCH - PT_COLS + 1) return false;
  const int a = dgrad ? (g.kh + g.sh - 1) / g.sh : g.kh;
  const int rows = (PT_ROWS - 1) * (dgrad ? 1 : g.sh) + a + 1;
  const int taps = ((a * g.kw) + 1) & ~1;
  if (rows > PT_PROWS || taps > PT_TMAX) return false;
  if (!fits_buf32(dgrad ? (int64_t)g.ho * g.wo : (int64_t)g.hi * g.wi)) return false;
  const int M = dgrad ? g.ci : g.co, L = dgrad ? g.co : g.ci;
  const int mb = (M + 31) / 32;
  p = ConvPlan{};
  p.rung = dgrad ? DS2_CONV_DG_PATCH : DS2_CONV_FWD_PATCH;
  p.tstride = wimg_tstride(g, dgrad);
  p.img = (int64_t)(dgrad ? g.sh : 1) * mb * L * wimg_tile(p.tstride);
  p.ws_bytes = (size_t)p.img * sizeof(float);
  p.gx = cdiv(dgrad ? g.wi : g.wo, PT_COLS);
  if (!dgrad) {
    p.gy = cdiv(g.ho, PT_ROWS);
  } else {
    for (int q = 0, hq; q < g.sh; ++q) p.gy += cdiv(class_rows(g, q, &hq), PT_ROWS);
  }
  plan_grid(p, (int64_t)g.n * mb);
  return true;
}

// the single-channel patch forward (conv1_patch_fwd_kernel): one input channel, <= 32 output
// channels, 3 <= kw <= 12, a patch and filter bank that fit its LDS
static inline bool plan_c1(const ConvDims& g, ConvPlan& p) {
  if (g.ci != 1 || g.co > 32 || g.kw < 3 || g.kw > 12) return false;
  const int kw2 = (g.kw + 1) & ~1;
  const int64_t pe = (int64_t)((C1_RW - 1) * g.sh + g.kh) * ((C1_WC - 1) * g.sw + kw2);
  if (pe > C1_PATCH || g.kh * kw2 > C1_KROWS) return false;
  p = ConvPlan{};
  p.rung = DS2_CONV_FWD_C1;
  p.a = kw2 / 2;
  p.gx = cdiv(g.wo, C1_WC);
  p.gy = cdiv(g.ho, C1_RW);
  plan_grid(p, g.n);   // tiles; the launch caps the workgroups at one per CU
  return true;
}

static inline ConvPlan conv_plan_fwd(const ConvDims& g, const ConvSwitches& s) {
  ConvPlan p;
  if (plan_x6(g, s, false, p) || plan_patch(g, false, p) || plan_c1(g, p)) return p;
  p = ConvPlan{};
  p.rung = DS2_CONV_FWD_GEMM;
  return p;
}

static inline ConvPlan conv_plan_dgrad(const ConvDims& g, const ConvSwitches& s) {
  ConvPlan p;
  if (plan_x6q(g, s, p) || plan_x6(g, s, true, p) || plan_patch(g, true, p)) return p;
  p = ConvPlan{};
  p.rung = DS2_CONV_DG_GEMM;
  return p;
}

// ds2_conv2d_workspace_size: every family of both directions that takes the shape
static inline size_t conv_ws_max(const ConvDims& g, const ConvSwitches& s) {
  ConvPlan p;
  size_t m = 0;
  if (plan_x6(g, s, false, p)) m = std::max(m, p.ws_bytes);
  if (plan_patch(g, false, p)) m = std::max(m, p.ws_bytes);
  if (plan_x6q(g, s, p)) m = std::max(m, p.ws_bytes);
  if (plan_x6(g, s, true, p)) m = std::max(m, p.ws_bytes);
  if (plan_patch(g, true, p)) m = std::max(m, p.ws_bytes);
  return m + 256;
}

// Weight gradient.  bf16x6 / fp16x3 (conv_x6_wgrad_sw_kernel, conv_x6_wgrad_kernel): width
// stride 1, the instantiated kernel columns (kw 11, pw 5), <= 32 channels each side, channel
// stacks within 32-bit buffer offsets; the sliding window for row strides <= 2 (8 tap rows
// per group, one workgroup per CU), per-row re-staging otherwise (4).  fp32 LDS tiles
// (conv_wgrad_patch_kernel): width stride 1 or 2, NT 2 or 4 tap tiles per wave by the x patch
// that fits.  Else the implicit GEMM, one partial slab per sample.
static inline ConvPlan conv_plan_wgrad(const ConvDims& g, const ConvSwitches& s) {
  ConvPlan p;
  const size_t per = (size_t)g.co * g.ci * g.kh * g.kw * sizeof(float);
  if (s.x6 && g.sw == 1 && g.kw == 11 && g.pw == 5 && g.ci <= 32 && g.co <= 32 &&
      fits_buf32((int64_t)g.co * g.ho * g.wo) && fits_buf32((int64_t)g.ci * g.hi * g.wi)) {
    const int64_t Rsw = (int64_t)g.n * ((g.wo + SW_COLS - 1) / SW_COLS) * g.ho;
    const bool sliding = g.sh <= 2 && Rsw < (1ll << 31) - 1;
    const int nw = sliding ? 8 : 4;
    const int G = (g.kh + nw - 1) / nw;
    const int64_t R = sliding ? Rsw : (int64_t)g.n * g.ho;
    const int64_t S = std::max<int64_t>(1, (nw == 8 ? CW_SLOTS / 2 : CW_SLOTS) / G);
    p.rung = !sliding ? DS2_CONV_WG_X6_ROW : !s.h3w ? DS2_CONV_WG_X6_SW
             : s.w64 ? DS2_CONV_WG_H3_SW64 : DS2_CONV_WG_H3_SW32;
    p.h3 = sliding && s.h3w;
    p.a = nw;
    p.b = G;
    p.splits = static_cast<int>(std::min(S, R));
    p.grid = (int64_t)G * p.splits;
    // the partial blocks, then the fp16x3 channel maxima (co, then ci), 256-B aligned
    p.co_amax = conv_align256((size_t)p.splits * G * (X6W_BLOCK / 4 * nw) * g.kw * sizeof(float));
    p.ci_amax = p.co_amax + (size_t)g.co * 4;
    p.ws_bytes = p.ci_amax + (size_t)g.ci * 4 + 512;
    return p;
  }
  p.rung = DS2_CONV_WG_GEMM;
  p.ws_bytes = (size_t)g.n * per + 256;
  if (g.sw > 2) return p;                  // kernels instantiated for width stride 1 and 2
  const int T = g.kh * g.kw;
  const int prow = (WG_RW - 1) * g.sh + g.kh;
  const int pcol = (WG_CW - 1) * g.sw + g.kw;
  // x patch row pitch == 11 mod 32 spreads the 3 tap rows of a tile over banks
  const int pitch = pcol + ((11 - pcol % 32) + 32) % 32;
  if (!fits_buf32(32 * (int64_t)g.ho * g.wo) || !fits_buf32((int64_t)g.hi * g.wi)) return p;
  if (T <= 8 * 32 && prow * pitch <= WG_XS_SMALL) {
    p.a = 2;
  } else if (T <= 16 * 32 && prow * pitch <= WG_XS_LARGE) {
    p.a = 4;
  } else {
    return p;
  }
  p.rung = DS2_CONV_WG_PATCH;
  p.b = g.sw;
  p.pitch = pitch;
  // one round of equal workgroups: 2 per CU (80 KB of LDS each at NT 4) x 256 CUs; the
  // bands split each sample's chunk list evenly (conv1: 32 x 16 bands of 10-11 chunks)
  const int64_t wgs = (int64_t)g.n * g.ci * ((g.co + 31) / 32);
  const int nck = ((g.ho + WG_RW - 1) / WG_RW) * ((g.wo + WG_CW - 1) / WG_CW);
  const int bands = wgs > 0 ? static_cast<int>((512 + wgs / 2) / wgs) : 1;
  p.bands = bands < 1 ? 1 : (bands > nck ? nck : bands);
  p.grid = (int64_t)p.bands * wgs;
  p.ws_bytes = (size_t)g.n * p.bands * per + 256;
  return p;
}

// --- conv_split.hip: the bf16x6 / fp16x3 launches of the plans' rungs ------------------------
// forward (in = x, out = y) and dgrad (in = dy, out = dx; no bias, no lengths)
ds2_status_t launch_conv_split(const ConvPlan& p, const ConvDims& g, const float* in,
                               const float* w, const float* bias, float* out, const int* out_lens,
                               void* ws, hipStream_t st);
// the partial blocks and their reduction into dw (not the bias gradient)
ds2_status_t launch_conv_split_wgrad(const ConvPlan& p, const ConvDims& g, const float* dy,
                                     const float* x, float* dw, void* ws, hipStream_t st);

}  // namespace ds2
