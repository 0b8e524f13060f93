// Host side of the recurrent dispatch (gru.hip, gru_split.hip, gru_xl.hip, lstm.hip): the
// environment switches, the shape counts, the workspace carve-up, the instance tables'
// lookup, the argument structs of the internal launchers and the single declaration of every
// function one of those files defines and another calls.  DESIGN.md "Recurrent dispatch" has
// the ladder per cell type and the table of switches.
// rnn.hip (the per-step tanh RNN) stays outside: it calls nothing from here, its two entry
// points are declared in ds2hip.h, and rnn_common.h would add err_fold_kernel to its device code.
#pragma once

#include "rnn_common.h"

#include <algorithm>
#include <cstddef>

namespace ds2 {

// --- environment switches: read at every call, never cached (the tests flip them) ---------
// first character of the variable as a digit, -1 when unset or not a digit
static inline int env_digit(const char* name) {
  const char* e = getenv(name);
  return (e != nullptr && e[0] >= '0' && e[0] <= '9') ? e[0] - '0' : -1;
}
// every on/off switch is on unless its variable starts with '0'
static inline bool env_off(const char* name) { return env_digit(name) == 0; }

static inline bool persistent_enabled() { return !env_off("DS2_RNN_PERSISTENT"); }
// DS2_GRU_STAMPS: 1 = phase stamps, 2 = the per-step trace window (a larger counter region)
static inline int stamp_mode() {
  const int m = env_digit("DS2_GRU_STAMPS");
  return m == 1 || m == 2 ? m : 0;
}

// --- shape ---------------------------------------------------------------------------------
struct RnnShape {
  int t, n, h, d;   // steps, samples, hidden units, directions
  int UB() const { return (h + GU - 1) / GU; }                           // 16-unit blocks
  int BT(int samples = GB) const { return (n + samples - 1) / samples; } // batch tiles
  // hand-off groups: one per (direction, batch tile)
  int groups(int samples = GB) const { return d * BT(samples); }
  // byte offsets into a [t][n][d][gates h] fp32 array fit 32 bits (the persistent kernels)
  bool fits32(int gates) const { return (int64_t)t * n * d * gates * h * 4 < (1ll << 31); }
};

// Grid over UB unit blocks x BT batch tiles x D directions: the same-XCD groups
// (map_work_xgrp; DS2_GRU_XCD=0 switches them off) where the groups tile the 8 XCDs, else
// map_work's interleaved layout.  *same_xcd (nullable) is the kernels' flag argument.
static inline int group_grid(int UB, int BT, int D, int* same_xcd = nullptr) {
  const bool x = !env_off("DS2_GRU_XCD") && xgrp_fits(UB, BT, D);
  if (same_xcd != nullptr) *same_xcd = x ? 1 : 0;
  return x ? xgrp_grid(UB, BT, D) : mapped_grid(UB * D, BT);
}

// --- instance tables -----------------------------------------------------------------------
// {K, kernel} in ascending K; the smallest instantiated K >= need runs (what exceeds the need
// is predicated off), nullptr when none covers it
struct Instance {
  int k;
  const void* fn;
};
template <typename F>
static inline Instance inst(int k, F* f) { return Instance{k, reinterpret_cast<const void*>(f)}; }
template <size_t N>
static inline Instance pick_instance(const Instance (&table)[N], int need) {
  if (need >= 1)
    for (const Instance& e : table)
      if (need <= e.k) return e;
  return Instance{0, nullptr};
}

// --- workspace carve-up --------------------------------------------------------------------
// Regions are taken in order, each rounded up to 256 bytes, so `end` after the last take is
// the workspace size by construction.
struct Carve {
  size_t end = 0;
  size_t take(size_t bytes) {
    const size_t at = end;
    end = at + align256(bytes);
    return at;
  }
};
template <typename T>
static inline T* ws_at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

// The error word of a launch sits right behind its group counters: `groups` is the group
// count OF THAT LAUNCH (directions x the batch tiles the launch covers, in the launch's own
// samples per tile), not of the whole batch or of the workspace's sizing.
static inline unsigned* err_word(unsigned* ctrs, int groups) { return ctrs + groups; }

// the dynamic LDS of the direct-operand kernels: one workgroup per CU
constexpr unsigned kDopPadLds = 80 * 1024;

// --- arguments of the internal launchers ---------------------------------------------------
// (shape, tensors, hand-off, stream); passed by value, the kernel argument arrays point into
// the copies
struct RecFwd {
  const float* xproj;
  const float *w_hh_f, *w_hh_r, *b_hh_f, *b_hh_r;
  const int* lens;
  float* h_all;
  float* c_all;   // LSTM only
  float* gates;   // nullable (no cache: inference, the one-gate RNN)
  // the initial state (ds2_*_fwd_state): all NULL, or all set (c0: LSTM only) with one direction
  const float *h0 = nullptr, *c0 = nullptr, *hproj0 = nullptr;
  bool stateful() const { return h0 != nullptr; }
  FwdState state() const { return FwdState{h0, c0, hproj0}; }
};
struct RecBwd {
  const float* dy;
  int dy_dirs;
  const float *w_hh_f, *w_hh_r;
  const float* state;   // h_all (GRU, RNN) or c_all (LSTM)
  const float* gates;
  const int* lens;
  float *dgx, *dgh;     // dgh: GRU only
  double* dbp;          // bias-gradient partials, nullable
  unsigned* camax;      // column maxima of dgx / dgh, nullable
  float* rowp;          // row-maximum partials of dgx (XCD-local backward), nullable
};
struct Handoff {
  float* ring;
  unsigned* ctrs;
  size_t ctr_bytes;     // the counter region [ctrs, + ctr_bytes)
  unsigned* err;        // err_word(ctrs, groups of this launch)
  unsigned* err_out;    // the caller's status word, nullable
  unsigned long long* stamps;
  size_t lds_pad;
};

// What a launch is to the launch record (ds2_test_rnn_last_launch): the ladder's rung, the
// table entry's key (k; c: kBwdPersist's chunks), 16-sample tiles per workgroup, same-XCD flag
struct Ran {
  int rung, k, c, bts, same_xcd;
};
// every recurrence launch of the ladders goes through here: the record is written where the
// launch went out, by the code that chose the kernel
static inline bool launch_rec(const void* fn, const Ran& r, dim3 grid, dim3 block, void** args,
                              size_t lds, hipStream_t st) {
  if (fn == nullptr || rnn_launch(fn, grid, block, args, lds, st) != hipSuccess) return false;
  rnn_rec_launch(r.rung, r.k, r.c, r.bts, (int)(grid.x * grid.y * grid.z), r.same_xcd);
  return true;
}
// a kernel picked from a table, launched as the persistent kernels are (rnn_launch)
static inline bool launch_fn(const Instance& e, int rung, int bts, int same_xcd, int grid,
                             int block, void** args, size_t lds, hipStream_t st) {
  return launch_rec(e.fn, Ran{rung, e.k, 0, bts, same_xcd}, dim3(grid), dim3(block), args, lds, st);
}
// one launch of a per-step kernel (plain launch, no LDS pad); failures surface in launch_status
static inline void launch_step(const Instance& e, int grid, int block, void** args,
                               hipStream_t st) {
  if (hipLaunchKernel(e.fn, dim3(grid), dim3(block), args, 0, st) == hipSuccess)
    rnn_rec_launch(DS2_RUNG_PER_STEP, e.k, 0, 1, grid, 0);
}

// --- the fallback ladders ------------------------------------------------------------------
// zero the counter region; fill ring_fill bytes (0: none) of the ring with the sentinel
static inline bool reset_handoff(const Handoff& ho, size_t ring_fill, hipStream_t st) {
  if (hipMemsetAsync(ho.ctrs, 0, ho.ctr_bytes, st) != hipSuccess) return false;
  return ring_fill == 0 || hipMemsetAsync(ho.ring, 0xFF, ring_fill, st) == hipSuccess;
}

// One rung over the whole batch: run `launch` (after reset_handoff when `reset`; a rung that
// follows a declined one on the same hand-off state needs none).  True: the ladder ends here
// with *rc -- the launch went out and its error word is folded into err_out, or the reset
// failed.  False: declined or failed to launch; the HIP error is cleared, the next rung
// starts clean.
template <typename Launch>
static inline bool rung(const char* what, const Handoff& ho, bool reset, size_t ring_fill,
                        hipStream_t st, ds2_status_t* rc, Launch launch) {
  if (reset && !reset_handoff(ho, ring_fill, st)) {
    *rc = launch_status(what);
    return true;
  }
  if (!launch()) {
    (void)hipGetLastError();
    return false;
  }
  fold_err(ho.err, ho.err_out, st);
  *rc = launch_status(what);
  return true;
}

// A rung in batch chunks: launch(b0, bt, ho) for consecutive tile ranges [b0, b0 + bt) of at
// most `chunk` tiles, each after its own reset and with its own error word (D * bt groups).
// One rule: a failure after a successful chunk is an error, not a fallback -- part of the
// outputs is written.  (The loop stops at the first failure, so "a chunk succeeded before"
// and "b0 > 0" are the same test.)  Returns as rung does.
template <typename Launch>
static inline bool for_each_chunk(const char* what, Handoff ho, int D, int tiles, int chunk,
                                  size_t ring_fill, hipStream_t st, ds2_status_t* rc,
                                  Launch launch) {
  for (int b0 = 0; b0 < tiles; b0 += chunk) {
    const int bt = std::min(chunk, tiles - b0);
    ho.err = err_word(ho.ctrs, D * bt);
    const bool ok = reset_handoff(ho, ring_fill, st);
    if (ok && launch(b0, bt, ho)) {
      fold_err(ho.err, ho.err_out, st);
      continue;
    }
    if (ok && b0 == 0) {
      (void)hipGetLastError();
      return false;
    }
    break;
  }
  *rc = launch_status(what);
  return true;
}

// --- gru_split.hip: the 16-unit fp16x3 / bf16x6 family -------------------------------------
// `ng` is the gate count of the instantiation: 1 the tanh RNN, 3 the GRU, 4 the LSTM
// (backward only).  The grids are the launches' own choice, -1 where they decline the shape.
int fwd16_grid(int ng, RnnShape s);
int bwd16_grid(int ng, RnnShape s, int bt_launch);
bool launch_fwd16(int ng, RnnShape s, RecFwd a, Handoff ho, hipStream_t st);
// one launch over the 16-sample tiles [tile0, tile0 + bt_launch); *camax_fused (nullable):
// whether the kernel that ran leaves the column maxima in a.camax
bool launch_bwd16(int ng, RnnShape s, RecBwd a, Handoff ho, hipStream_t st, int tile0,
                  int bt_launch, bool* camax_fused);
size_t h3_bwd_ring_bytes(int n_tiles, int h, int num_dirs, int ng);
// the single-term LSTM backward (32-sample tiles)
int lstm_h1_grid(RnnShape s);
size_t lstm_h1_ring_bytes(int n, int h, int num_dirs);
bool launch_lstm_bwd_h1(RnnShape s, RecBwd a, Handoff ho, hipStream_t st);

// --- gru_xl.hip: the XCD-local groups (32 units x 8 samples per workgroup) ------------------
int gru_xl_groups(int n, int h, int num_dirs);
int gru_xl_active(int n, int h, int num_dirs);
size_t gru_xl_ctr_words();
bool launch_gru_fwd_xl(RnnShape s, RecFwd a, Handoff ho, hipStream_t st);
bool launch_gru_bwd_xl(RnnShape s, RecBwd a, Handoff ho, hipStream_t st);
size_t gru_xl_rowp_bytes(int t_max, int n, int h, int num_dirs);
void launch_gru_xl_row_amax(int t_max, int n, int h, int num_dirs, const float* rowp,
                            unsigned* out, hipStream_t st);

}  // namespace ds2
