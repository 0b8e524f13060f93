/*
 * libds2hip test hooks — NOT part of the product ABI (include/ds2hip.h).
 *
 * Entry points the GPU tests and profiling scripts use to observe the kernels from the
 * outside: holding CUs the way a collective's CTAs would, stamping the device clock, and
 * per-phase clock stamps of the beam search.  Nothing on the training or decoding path
 * calls them; they are exported from the same libds2hip.so so the tests exercise the
 * shipped binary.
 */
#ifndef DS2HIP_TEST_H
#define DS2HIP_TEST_H

#include "ds2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Residency test hooks (csrc/residency.hip; not on the training path).  ds2_test_occupy:
 * `ctas` one-wave workgroups with lds_kb KB of dynamic LDS each (> 80: alone on their CU,
 * no recurrence workgroup fits beside), each spinning for max_us microseconds on the
 * device clock, recording rec[4*i..4*i+3] = {start, end (s_memrealtime, 100 MHz),
 * XCC id, HW_ID}.  ds2_test_rnn_launch_lds: the same with 94 KB of static LDS launched
 * through the recurrences' launcher and its 80 KB pad (the pad must be clamped to fit).
 * ds2_test_timestamp: *out = s_memrealtime when the stream reaches it.         */
ds2_status_t ds2_test_occupy(int ctas, int lds_kb, int max_us, unsigned long long* rec,
                             ds2_stream_t stream);
ds2_status_t ds2_test_rnn_launch_lds(int ctas, int max_us, unsigned long long* rec,
                                     ds2_stream_t stream);
ds2_status_t ds2_test_timestamp(unsigned long long* out, ds2_stream_t stream);

/* ds2_test_ring_traffic: the local HBM traffic of a ring all-reduce of `count` fp32 values
 * over `world` ranks, on ONE GPU (DESIGN.md §6 interference measurement): 2 (world - 1)
 * phases, each reading a count / world chunk of `bucket` (never written) and of `scratch`
 * (>= count / world floats) and writing the scratch chunk, phase p starting p * (chunk bytes
 * / busbw) after the start (busbw_gbps = 0: unpaced), on `ctas` workgroups of 256 threads.
 * bucket and scratch 16-B aligned.                                                      */
ds2_status_t ds2_test_ring_traffic(const float* bucket, int64_t count, int world, float* scratch,
                                   int ctas, double busbw_gbps, ds2_stream_t stream);

/* ds2_test_beam_stamps: test hook; every later beam decode writes per-phase clock stamps of
 * utterance 0's first 256 frames into buf ([256][9] uint64: s_memtime at the 8 phase
 * boundaries of a frame, then s_memrealtime at its start); buf = NULL turns it off.       */
ds2_status_t ds2_test_beam_stamps(unsigned long long* buf);

/* ------------------------------------------------------------------------ */
/* ds2_test_rnn_last_launch: which kernel the recurrent entry point last called ON THIS THREAD
 * launched (ds2_gru_fwd, ds2_gru_bwd*, ds2_rnn_fwd[_ws], ds2_rnn_bwd[_ws], ds2_lstm_fwd,
 * ds2_lstm_bwd, ds2_lstm_bwd_half).  Host only: the record is reset at the entry point and
 * written where a recurrence launch went out, by the dispatch itself -- nothing recomputes
 * the choice.  out[7] =
 *   [0] rung: a DS2_RUNG_* value, a row of DESIGN.md's ladder table (NONE: nothing launched)
 *   [1] k: the instance key K of the table entry that ran (inst(K, ...); kBwdPersist's k;
 *       0 for the per-step tanh RNN kernels, which have no table)
 *   [2] c: kBwdPersist's chunk count, 0 elsewhere
 *   [3] bts: 16-sample tiles per workgroup (the single-term backward's 32-sample tiles: 2;
 *       the XCD-local kernels' 8-sample tiles: 0)
 *   [4] launches: recurrence launches that went out (batch chunks; t_max for per-step)
 *   [5] grid: workgroups of the first launch (x * y * z)
 *   [6] same_xcd: the same-XCD flag passed to the first launch (XCD-local: 1)           */
enum {
  DS2_RUNG_NONE = 0,
  DS2_RUNG_XCD_LOCAL = 1,    /* gru_xl.hip */
  DS2_RUNG_H3_16 = 2,        /* 16-unit fp16x3 (GRU, one-gate RNN, four-gate LSTM backward) */
  DS2_RUNG_X6_16 = 3,        /* 16-unit bf16x6 (GRU) */
  DS2_RUNG_DOP = 4,          /* direct-operand: fp32 MFMA (GRU; LSTM forward, DS2_LSTM_H3=0) */
  DS2_RUNG_DOP_H3 = 5,       /* direct-operand fp16x3 (LSTM forward) */
  DS2_RUNG_LDS_PERSIST = 6,  /* LDS-staged persistent */
  DS2_RUNG_SINGLE_TERM = 7,  /* single-term fp16 LSTM backward (ds2_lstm_bwd_half) */
  DS2_RUNG_PER_STEP = 8      /* one launch per step */
};
ds2_status_t ds2_test_rnn_last_launch(int* out);

/* ------------------------------------------------------------------------ */
/* ds2_test_conv2d_plan: what ds2_conv2d_fwd (dir 0), ds2_conv2d_dgrad (1) or ds2_conv2d_wgrad
 * (2) would launch for the shape under the current DS2_CONV_* environment.  Host only, no
 * device needed, nothing launched: it calls the function the entry point switches on
 * (csrc/conv_host.h conv_plan_*).  DS2_INVALID_VALUE for a shape the entry point rejects.
 * out[11] =
 *   [0] rung: a DS2_CONV_* value, a row of DESIGN.md's conv dispatch table
 *   [1] [2] its parameters: FWD_C1 KWH, 0; WG_PATCH NT, SW; the WG_H3 / WG_X6 rungs: tap rows
 *       per group, groups; 0 elsewhere
 *   [3] [4] workspace bytes the rung needs, low and high 32 bits
 *   [5] gx: column tiles           [6] gy: rows / row pairs / row tiles
 *   [7] splits  [8] bands  [9] x patch pitch (wgrad; 0 elsewhere)
 *   [10] workgroups of the convolution kernel (FWD_C1: tiles), saturating at INT_MAX;
 *        0 for the implicit-GEMM rungs (3-D grids)                                    */
enum {
  DS2_CONV_NONE = 0,
  DS2_CONV_FWD_H3_2R = 1,        /* conv_h3_fwd2r_kernel */
  DS2_CONV_FWD_H3_1R = 2,        /* conv_x6_kernel<false, 3, 6, 2, 1, false, true, 2> */
  DS2_CONV_FWD_X6_DB = 3,        /* conv_x6_kernel<false, 3, 6, 2, 1, false, true> */
  DS2_CONV_FWD_X6 = 4,           /* conv_x6_kernel<false, 0, 0, 3, 0, true> */
  DS2_CONV_FWD_PATCH = 5,        /* conv_patch_kernel<false> */
  DS2_CONV_FWD_C1 = 6,           /* conv1_patch_fwd_kernel<KWH> */
  DS2_CONV_FWD_GEMM = 7,         /* conv_fwd_kernel */
  DS2_CONV_DG_H3_2R = 8,         /* conv_h3_dgrad2r_kernel */
  DS2_CONV_DG_H3_Q = 9,          /* conv_x6q_dgrad_kernel<true, 2, true> */
  DS2_CONV_DG_H3_Q_NOFLUSH = 10, /* conv_x6q_dgrad_kernel<true, 2, false> */
  DS2_CONV_DG_X6_Q = 11,         /* conv_x6q_dgrad_kernel<true, 3> */
  DS2_CONV_DG_X6_26 = 12,        /* conv_x6_kernel<true, 2, 6, 2, 1, false> */
  DS2_CONV_DG_X6 = 13,           /* conv_x6_kernel<true, 0, 0, 3, 0, true> */
  DS2_CONV_DG_PATCH = 14,        /* conv_patch_kernel<true> */
  DS2_CONV_DG_GEMM = 15,         /* conv_dgrad_kernel */
  DS2_CONV_WG_H3_SW32 = 16,      /* conv_x6_wgrad_sw_kernel<11, 3, 8, 2> */
  DS2_CONV_WG_H3_SW64 = 17,      /* conv_x6_wgrad_sw_kernel<11, 3, 8, 2, 64> */
  DS2_CONV_WG_X6_SW = 18,        /* conv_x6_wgrad_sw_kernel<11, 3, 8> */
  DS2_CONV_WG_X6_ROW = 19,       /* conv_x6_wgrad_kernel<11, 3> */
  DS2_CONV_WG_PATCH = 20,        /* conv_wgrad_patch_kernel<NT, XS, SW> */
  DS2_CONV_WG_GEMM = 21          /* conv_wgrad_kernel */
};
ds2_status_t ds2_test_conv2d_plan(int dir, int n, int c_in, int h_in, int w_in, int c_out, int kh,
                                  int kw, int sh, int sw, int ph, int pw, int* out);

/* ------------------------------------------------------------------------ */
/* ds2_test_conv1d_plan: what ds2_conv1d_fwd (dir 0), ds2_conv1d_dgrad (1) or ds2_conv1d_wgrad
 * (2) would launch for the shape under the current DS2_CONV1D.  Host only, no device needed,
 * nothing launched: it calls the function the entry points switch on (csrc/conv1d.hip
 * c1_plan).  dir + 4: the same for ds2_conv1d_fwd_amax / ds2_conv1d_wgrad_amax with the
 * maxima supplied (dgrad: no such entry, as dir 1).  x_addr: the address of the gathered
 * activations (forward: x, dgrad: dy; ignored by wgrad); only its low four bits are used.
 * Returns DS2_INVALID_VALUE or DS2_UNSUPPORTED_SHAPE exactly where the entry point does before
 * it looks at a pointer.  out[10] =
 *   [0] path: a DS2_C1_* value, a row of DESIGN.md's Conv1d dispatch table (NONE: an empty
 *       call: forward and dgrad launch nothing, wgrad zero-fills dw and dbias)
 *   [1] stages of the implicit GEMM, k * pad32(channels of the gathered operand) / 32; else 0
 *   [2] [3] [4] grid x, y, z of the convolution kernel (GEMM: 0, ds2_sgemm_ws plans its own)
 *   [5] nsplit  [6] kchunk: the slabs of the fp16x3 wgrad's K = t_out n (else 0)
 *   [7] [8] workspace bytes the entry point checks for before it launches, low and high 32
 *       bits (never more than the size query); 0: the path takes NULL
 *   [9] row-maxima (implicit GEMM) or column-maxima (WGRAD_H3) passes launched            */
enum {
  DS2_C1_NONE = 0,
  DS2_C1_GEMM = 1,          /* k = 1, s = 1, p = 0: ds2_sgemm_ws */
  DS2_C1_IGEMM_VEC = 2,     /* c1_igemm_kernel<true>: float4 loads of the activations */
  DS2_C1_IGEMM_SCALAR = 3,  /* c1_igemm_kernel<false> */
  DS2_C1_WGRAD_H3 = 4,      /* c1_wgrad_kernel + c1_wgrad_reduce_kernel */
  DS2_C1_GENERAL = 5        /* c1_general_kernel<dir> */
};
ds2_status_t ds2_test_conv1d_plan(int dir, int t, int n, int c_in, int c_out, int k, int s, int p,
                                  unsigned long long x_addr, int* out);

/* ------------------------------------------------------------------------ */
/* ds2_test_sgemm_plan: what ds2_sgemm / ds2_sgemm_ws / ds2_sgemm_amax_ws (kind 0),
 * ds2_sgemm_bf16_ws (kind 1) or ds2_bgemm_nt (kind 2: trans and batch ignored, ld in bf16
 * elements) would launch under the current DS2_GEMM_* environment.  Host only, no device
 * needed (with cus > 0), nothing launched: it calls the function the entry points switch on
 * (csrc/gemm_host.h gemm_select).  a, b, c, bias: the addresses as integers; only their low
 * four bits are used, and whether they are 0.  have_ws / ws_bytes: the workspace the call
 * passes.  amax_given: bit 0 / 1, the caller supplies the row maxima of op(A) / op(B).
 * cus: the CU count the plan is made for (0: the current device's).  Returns DS2_OK whatever
 * the call would return; out[14] =
 *   [0] rung: a DS2_GEMM_* value, a row of DESIGN.md's GEMM dispatch table (NONE: nothing
 *       launched -- an empty product or a rejected call)
 *   [1] bm  [2] bn: the tile
 *   [3] main_wgs: whole-tile workgroups   [4] tail_tile0  [5] tail_tiles
 *   [6] nsplit  [7] kchunk: the K split of the tail tiles
 *   [8] grid: workgroups of the GEMM kernel, main_wgs + tail_tiles * batch * nsplit
 *   [9] [10] workspace bytes the rung uses, low and high 32 bits
 *   [11] vec: the 16-byte form of the split reduce (bgemm: of the C rows)
 *   [12] status: what the entry point returns before any launch
 *   [13] row-maxima passes launched ahead of the GEMM (fp16x3 without caller maxima: 2) */
enum {
  DS2_GEMM_NONE = 0,
  DS2_GEMM_H3_160 = 1,       /* sxgemm2_kernel<TA, TB, false, 160, 2, true>: fp16x3 */
  DS2_GEMM_H3_128 = 2,       /* sxgemm2_kernel<TA, TB, false, 128, 2, true> */
  DS2_GEMM_X6_M16_160 = 3,   /* sxgemm2_kernel<TA, TB, false, 160, 3, true>: bf16x6 16x16x32 */
  DS2_GEMM_X6_M16_128 = 4,   /* sxgemm2_kernel<TA, TB, false, 128, 3, true> */
  DS2_GEMM_X6_160 = 5,       /* sxgemm2_kernel<TA, TB, false, 160, 3, false>: 32x32x16 */
  DS2_GEMM_X6_128 = 6,       /* sxgemm2_kernel<TA, TB, false, 128, 3, false> */
  DS2_GEMM_X6_K_160 = 7,     /* sxgemm2_kernel<TA, TB, true, 160, 3, false>: k checked */
  DS2_GEMM_X6_K_128 = 8,     /* sxgemm2_kernel<TA, TB, true, 128, 3, false> */
  DS2_GEMM_F64_160 = 9,      /* sgemm64_kernel<TA, TB, 5, 64, 1>: fp32 MFMA, BK = 64 */
  DS2_GEMM_F64_128 = 10,     /* sgemm64_kernel<TA, TB, 4, 64, 1> */
  DS2_GEMM_F16 = 11,         /* sgemm_kernel<TA, TB, VA, VB>: fp32 MFMA, BK = 16 */
  DS2_GEMM_BF16_STAGED = 12, /* sbgemm_kernel<TA, TB> (ds2_sgemm_bf16_ws) */
  DS2_GEMM_BF16_DMA = 13,    /* bgemm_nt_kernel<false> (ds2_bgemm_nt) */
  DS2_GEMM_BF16_DMA_K = 14   /* bgemm_nt_kernel<true>: k checked */
};
ds2_status_t ds2_test_sgemm_plan(int kind, int trans_a, int trans_b, int m, int n, int k,
                                 unsigned long long a, int64_t lda, int64_t stride_a,
                                 unsigned long long b, int64_t ldb, int64_t stride_b,
                                 unsigned long long c, int64_t ldc, int64_t stride_c, int batch,
                                 unsigned long long bias, int have_ws, size_t ws_bytes,
                                 int amax_given, int cus, int* out);

/* ds2_test_sgemm_cover: runs every workgroup id in [0, grid) through the kernels' own work
 * decode (csrc/gemm_host.h decode_work / tile_coords; bg_decode for 256 x 256 tiles) on the
 * host and returns the number of (batch, tile) pairs whose pieces do not partition [0, k)
 * exactly once plus the number of decoded tiles outside the tile grid (a correct plan: 0);
 * -1 for arguments no plan has (a non-positive size, grid < main_wgs).          */
long long ds2_test_sgemm_cover(int m, int n, int k, int batch, int bm, int bn, int main_wgs,
                               int tail_tile0, int tail_tiles, int nsplit, int kchunk, int grid);

#ifdef __cplusplus
}
#endif

#endif /* DS2HIP_TEST_H */
