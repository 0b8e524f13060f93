// GRU recurrences in XCD-local hand-off groups (round 6; default where the shape fits).
//
// The fp16x3 kernels of gru_split.hip tile a (direction, 16-sample) group as 50 workgroups of
// 16 units at cfg2 (H 800).  A group then spans two XCDs, and every step each consumer pulls
// 50 producer tiles (the backward: 50 x 3.06 KB = 153 KB), half of them across the fabric
// (MI355X_MICROARCH "handoff-payload": 62-70 GB/s per block cross-XCD, 104-122 same-XCD from
// plain stores).  The backward's no-synchronisation bound was 4.02 us of its 5.0 us step: the
// bytes, not the protocol, set the step.
//
// Here a workgroup owns 32 units x 8 samples, so a group is H / 32 = 25 workgroups (one XCD's
// 32 CUs) and cfg2 runs 2 directions x 4 batch tiles = 8 groups, one per XCD (200 workgroups).
// Per step a consumer pulls 25 forward tiles of 1 KB (was 50) or 25 backward records of
// 3.1 KB (was 153 KB), all from its own XCD's L2.
//
// Which XCD a workgroup runs on is never assumed: every workgroup publishes its HW_REG_XCC_ID
// at start (agent-scope atomic store) and waits for its group's ids.  If all share one XCD the
// group runs LOCAL: payloads and flags are stored plainly (they stay in that XCD's L2, the
// coherence point of its CUs) and read with sc1 loads (L1 bypassed, served by that L2).  Else
// the group runs GLOBAL: every store is sc1 (write-through) and the protocol is
// MI355X_MICROARCH "Valid forms" row 1, correct at any placement.  Blocks b with equal b % 8
// form a group, which under the observed round-robin dispatch lands on one XCD.
//
// Half-empty 16-row MFMAs are avoided by stacking: an A fragment holds the fp16 hi terms of
// the 8 samples in rows 0-7 and their lo terms in rows 8-15, so A.W_hi gives hi.W_hi (rows
// 0-7) and lo.W_hi (rows 8-15) and A.W_lo gives hi.W_lo (rows 0-7; rows 8-15 = lo.lo): the
// three fp16x3 products in two v_mfma_f32_16x16x32_f16, and the big (hi.hi) and small products
// land in different rows, i.e. in separate accumulation chains (the MFMA rounding note of
// DESIGN.md section 4).  The two halves are added when the waves' partials are reduced.
// Producers publish these stacked fragments ready-made (the forward's 1-KB tile is exactly the
// fp16 A fragment of its 8 x 32 h values), so consumers load one 16-B run per lane per tile
// and split nothing.
//
// Forward hand-off: the sentinel ring of gru_fwd_x6_kernel (4 slots, the data is the flag),
// tiles consumed in a fixed producer order (a wave multiplies tile p only after tile p - 1:
// deterministic sums).  Backward: per-producer flags (the record after a drain, then the
// flag), each wave waiting for the flags of its own producers only; records multiplied in a
// fixed order, three in flight per wave beside the one multiplied.
#include "rnn_host.h"

#include <algorithm>

namespace ds2 {

// Timing ablations (scripts/xl_ablation.sh builds them into deepspeech.pytorch_amd/ablation/;
// results wrong, never in the product library): bit 0 skips the per-step pointwise input loads
// (xproj; dy / gates / h_prev), bit 1 the per-step output stores (h_all / gates; dgx / dgh),
// bit 2 every hand-off wait (the tiles / records are read whatever they hold).
#ifndef DS2_XL_ABL
#define DS2_XL_ABL 0
#endif
constexpr bool kAblLoads = (DS2_XL_ABL & 1) != 0;
constexpr bool kAblStores = (DS2_XL_ABL & 2) != 0;
constexpr bool kAblWait = (DS2_XL_ABL & 4) != 0;
constexpr bool kAblFixT = (DS2_XL_ABL & 8) != 0;   // every step loads the rows of t = 0

constexpr int LB = 8;            // samples per workgroup
constexpr int LU = 32;           // units per workgroup
constexpr int LW = 4;            // waves per workgroup, one per SIMD (the whole register file)
constexpr int LT = LW * 64;      // 256 threads = 8 samples x 32 units, one owner each
constexpr int LSLOTS = 4;        // forward sentinel ring slots
constexpr int LRB = 784;         // floats per backward record: 3 x 1-KB fragments + 8 factors
constexpr int kXlTraceS0 = 100, kXlTraceSteps = 16;   // = gru.hip's DS2_GRU_STAMPS=2 window

// the launch's workgroup -> (group, producer index); blocks with equal b % 8 form a group
__device__ __forceinline__ bool xl_map(int G, int UBX, int& g, int& ub) {
  g = blockIdx.x & 7;
  ub = blockIdx.x >> 3;
  return g < G && ub < UBX;
}

// What only the cold paths read -- the error words a timed-out wait raises, the tensor and shape
// the poison fill needs -- parked in LDS by thread 0 at kernel start (the barrier of
// xl_group_local publishes it).  The step loop then holds none of it in SGPRs: at one wave per
// SIMD the loops ran out of them, and every spill reload (v_readlane) sat on the step's serial
// path.  (The loop's barriers and memory clobbers keep these loads where they are written.)
// The pointers keep their global address space: a pointer loaded back from LDS is generic, its
// atomics are FLAT, and with a FLAT access possibly outstanding the compiler turns every
// counted vmcnt(N) wait of the step loop into vmcnt(0) (the record loads then no longer overlap
// the products: 1.77 -> 1.82 ms per backward launch).
typedef __attribute__((address_space(1))) unsigned xl_gu32;
typedef __attribute__((address_space(1))) float xl_gf32;
struct XlCold {
  xl_gu32 *err, *err_out;
  xl_gf32* out;    // the poison fill's tensor (h_all / dgx)
  int N, D, H;
  int n0, j0;      // the workgroup's first sample and unit
};

__device__ __forceinline__ void xl_raise(const XlCold& c) {
  xl_gu32 *e = c.err, *eo = c.err_out;
  __hip_atomic_fetch_or(e, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (eo != nullptr) __hip_atomic_fetch_or(eo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// poison_rest from the cold block: `width` floats per row in `groups` slices of H columns
__device__ __forceinline__ void xl_poison(const XlCold& c, int s, int T, bool rev, int d,
                                          int width_h, int groups) {
  const int n = c.n0 + (int)(threadIdx.x >> 5);
  poison_rest((float*)c.out, s, T, rev, c.N, c.D, n, d, c.H, c.j0 + (int)(threadIdx.x & 31),
              width_h * c.H, groups, n < c.N);
}

// Every workgroup publishes its XCC id (+1) into its group's table and waits for the group's
// UBX entries; true when all equal this workgroup's (every member reaches the same answer from
// the same table).  A timeout sets the error word and answers false.  `mode` (diagnostic, read
// by scripts/trace_gru.py): OR of 1 (a member ran LOCAL) / 2 (GLOBAL) per group.
__device__ __forceinline__ bool xl_group_local(unsigned* xtab, int ub, int UBX, unsigned* err,
                                               unsigned* err_out, int* lds_word, unsigned* mode,
                                               int force_global) {
  const unsigned mine = xcc_id() + 1u;
  if (threadIdx.x == 0) __hip_atomic_store(xtab + ub, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((threadIdx.x >> 6) == 0) {
    const int lane = threadIdx.x & 63;
    unsigned v = mine;
    bool ok = true;
    for (unsigned spins = 0;; ++spins) {
      v = lane < UBX ? __hip_atomic_load(xtab + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                     : mine;
      if (__ballot(v == 0u) == 0ull) break;
      if (spins > g_spin_limit) {
        if (lane == 0) raise_err(err, err_out);
        ok = false;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    const bool loc = ok && __ballot(v != mine) == 0ull && force_global == 0;
    if (lane == 0) {
      *lds_word = loc ? 1 : 0;
      __hip_atomic_fetch_or(mode, loc ? 1u : 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  return *lds_word != 0;
}

// voff: the lane's byte offset (loop-invariant where it can be), soff: the wave-uniform part
__device__ __forceinline__ void xl_store(u32x4 v, __amdgpu_buffer_rsrc_t rs, int voff, int soff,
                                         bool local) {
  if (local)
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff, soff, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff, soff, kSc1);
}

// The waves' partial sums on their way to the owners.  An accumulator register holds the hi
// products' row m (< 8) in lane L < 32 and the lo products' row m + 8 in lane L + 32, and the
// owner adds exactly that pair first -- so the producing wave adds it (the same add, the same
// bits) before anything is written: one 32-lane swap per pair of registers (a: unit half 0, b:
// unit half 1) leaves a's pair in the two operands of lanes 0-31 and b's in those of lanes
// 32-63.  Half the LDS bytes written, half the reads per owner.
__device__ __forceinline__ float xl_fold(float a, float b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a),
                                                  __builtin_bit_cast(unsigned, b), false, false);
  // (the elements into scalars first: a bit cast applied to r[1] directly reads element 0)
  const unsigned r0 = r[0], r1 = r[1];
  return __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
}
// Folded partials in LDS: [wave][gate] blocks of 8 sample rows x 32 units, the unit's bit 4
// flipped in rows 4-7 (a wave writes rows i and 4 + i of 16 + 16 units at once: 32 banks).
// Where a lane writes its value of row 4 ((lane >> 4) & 1) + i: xl_fold_at(lane) + 32 i
__device__ __forceinline__ int xl_fold_at(int lane) {
  const int hi4 = (lane >> 4) & 1;
  return hi4 * 128 + (((lane & 15) + 16 * (lane >> 5)) ^ (16 * hi4));
}
// where the owner of (sample m, unit u) reads it
__device__ __forceinline__ int xl_fold_own(int m, int u) { return m * 32 + (u ^ ((m >> 2) << 4)); }

// max of v over the lane's half of the wave (lanes 0-31 / 32-63: one sample's 32 units), in
// every lane: four DPP steps inside each row of 16 (quad swaps, half-row and row mirrors),
// then the two rows of a half joined through readlane -- no LDS-crossbar shuffles (five
// dependent ds_bpermute, ~0.15 us, where this is ~40 cycles).  A maximum: the order is free.
#define DS2_DPP_MAX(v, ctrl)                                                               \
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(                      \
                   0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true)))
__device__ __forceinline__ float half_wave_max(float v) {
  DS2_DPP_MAX(v, 0xB1);    // quad_perm [1, 0, 3, 2]
  DS2_DPP_MAX(v, 0x4E);    // quad_perm [2, 3, 0, 1]
  DS2_DPP_MAX(v, 0x141);   // row_half_mirror
  DS2_DPP_MAX(v, 0x140);   // row_mirror
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (threadIdx.x & 32) ? fmaxf(r2, r3) : fmaxf(r0, r1);
}
#undef DS2_DPP_MAX

// The backward's per-wave flag wait: lane l polls the flag of the wave's producer l (`flags` =
// the group's flag line at the wave's first producer) until all `count` have reached `target`.
// The wave then loads those producers' records itself (MI355X_MICROARCH "Valid forms" row 1:
// the wave that polled loads after its own poll matched), without waiting for the group's
// other producers or for a workgroup barrier.  False, and the error words set, past the spin
// bound (DS2_RNN_SPIN_LIMIT=0: at once).
__device__ __forceinline__ bool xl_wave_flags_wait(const unsigned* flags, int count,
                                                   unsigned target, const XlCold& cold) {
  const int lane = threadIdx.x & 63;
  if (count == 0) return true;
  for (unsigned spins = 0;; ++spins) {
    if (spins > g_spin_limit || g_spin_limit == 0) {
      if (lane == 0) xl_raise(cold);
      return false;
    }
    const unsigned v = lane < count ? __hip_atomic_load(flags + lane, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT)
                                    : target;
    if (__ballot(v < target) == 0ull) return true;
    sleep_units(g_rnn_tune[3]);
  }
}

// W_hh fragments beyond the arch-VGPR budget stay in AGPRs for the whole kernel and the MFMAs
// read them there (gfx950 takes A / B operands from either half of the register file).  The
// compiler only ever parks a VGPR value in an AGPR as a spill and copies it back in front of
// every use (v_accvgpr_read: ~190 per forward step, ~310 per backward step at NPW 6), so these
// MFMAs are issued from inline asm whose operand constraints name the file: xl_agpr moves a
// fragment there once, at kernel start.  kXlVgprW: the producers whose fragments stay VGPRs.
constexpr int kXlVgprW = 2, kXlVgprWBwd = 1;
__device__ __forceinline__ u32x4 xl_agpr(u32x4 v) {
  u32x4 r;
  asm volatile("" : "=a"(r) : "0"(v));
  return r;
}
// What the compiler does not do for an asm statement: `s_nop 1` covers a VALU-written operand
// (a fragment or tile the allocator moved just before the statement), and whoever reads the
// accumulators next calls xl_mfma_settle first (the MFMA's result -> any other reader).  In
// the forward that is once per step, behind the last tile: between the tiles the accumulators
// are operands of the asm statements alone, and the compiler must not touch them there.  After
// a change, check the assembly (scripts/xl_reg_audit.py: no v_accvgpr_*, no spill; and no
// v_mov of an accumulator register between a step's first MFMA and the settle).
__device__ __forceinline__ void xl_mfma_settle(f32x4 (&c)[6]) {
  asm volatile("s_nop 15\n\ts_nop 7"
               : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]));
}
// One forward tile: c[ct] += a . lo[ct], then += a . hi[ct] (each c[ct] its own chain, small
// products first), the six chains interleaved.  WC: the fragments' register file.
#define DS2_XL_FWD_TILE(WC)                                                                  \
  asm volatile(                                                                              \
      "s_nop 1\n\t"                                                                          \
      "v_mfma_f32_16x16x32_f16 %0, %6, %7, %0\n\tv_mfma_f32_16x16x32_f16 %1, %6, %8, %1\n\t"  \
      "v_mfma_f32_16x16x32_f16 %2, %6, %9, %2\n\tv_mfma_f32_16x16x32_f16 %3, %6, %10, %3\n\t" \
      "v_mfma_f32_16x16x32_f16 %4, %6, %11, %4\n\tv_mfma_f32_16x16x32_f16 %5, %6, %12, %5\n\t" \
      "v_mfma_f32_16x16x32_f16 %0, %6, %13, %0\n\tv_mfma_f32_16x16x32_f16 %1, %6, %14, %1\n\t" \
      "v_mfma_f32_16x16x32_f16 %2, %6, %15, %2\n\tv_mfma_f32_16x16x32_f16 %3, %6, %16, %3\n\t" \
      "v_mfma_f32_16x16x32_f16 %4, %6, %17, %4\n\tv_mfma_f32_16x16x32_f16 %5, %6, %18, %5"      \
      : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5])               \
      : "v"(a), WC(lo[0]), WC(lo[1]), WC(lo[2]), WC(lo[3]), WC(lo[4]), WC(lo[5]), WC(hi[0]), \
        WC(hi[1]), WC(hi[2]), WC(hi[3]), WC(hi[4]), WC(hi[5]))
template <bool AG>
__device__ __forceinline__ void xl_fwd_tile(f32x4 (&c)[6], u32x4 a, const u32x4 (&lo)[6],
                                            const u32x4 (&hi)[6]) {
  if constexpr (AG)
    DS2_XL_FWD_TILE("a");
  else
    DS2_XL_FWD_TILE("v");
}
#undef DS2_XL_FWD_TILE

// One backward record: per unit half c the two zero-C chains c[2 c] (hi fragments) and
// c[2 c + 1] (lo) over the gates r, z, n, the four chains interleaved.  w[gate][half][hi, lo].
// The VALU adds the chains up right behind the statement, so the MFMA-result wait states are
// inside it (`s_nop 7` is what the compiler itself puts between this MFMA and a VALU reader).
#define DS2_XL_BWD_REC(WC)                                                                    \
  asm volatile(                                                                               \
      "s_nop 1\n\t"                                                                           \
      "v_mfma_f32_16x16x32_f16 %0, %4, %7, 0\n\tv_mfma_f32_16x16x32_f16 %1, %4, %8, 0\n\t"     \
      "v_mfma_f32_16x16x32_f16 %2, %4, %9, 0\n\tv_mfma_f32_16x16x32_f16 %3, %4, %10, 0\n\t"    \
      "v_mfma_f32_16x16x32_f16 %0, %5, %11, %0\n\tv_mfma_f32_16x16x32_f16 %1, %5, %12, %1\n\t" \
      "v_mfma_f32_16x16x32_f16 %2, %5, %13, %2\n\tv_mfma_f32_16x16x32_f16 %3, %5, %14, %3\n\t" \
      "v_mfma_f32_16x16x32_f16 %0, %6, %15, %0\n\tv_mfma_f32_16x16x32_f16 %1, %6, %16, %1\n\t" \
      "v_mfma_f32_16x16x32_f16 %2, %6, %17, %2\n\tv_mfma_f32_16x16x32_f16 %3, %6, %18, %3\n\t" \
      "s_nop 9"                                                                               \
      : "=&v"(c[0]), "=&v"(c[1]), "=&v"(c[2]), "=&v"(c[3])                                    \
      : "v"(ar), "v"(az), "v"(an), WC(w[0][0][0]), WC(w[0][0][1]), WC(w[0][1][0]),            \
        WC(w[0][1][1]), WC(w[1][0][0]), WC(w[1][0][1]), WC(w[1][1][0]), WC(w[1][1][1]),       \
        WC(w[2][0][0]), WC(w[2][0][1]), WC(w[2][1][0]), WC(w[2][1][1]))
template <bool AG>
__device__ __forceinline__ void xl_bwd_rec(f32x4 (&c)[4], u32x4 ar, u32x4 az, u32x4 an,
                                           const u32x4 (&w)[3][2][2]) {
  if constexpr (AG)
    DS2_XL_BWD_REC("a");
  else
    DS2_XL_BWD_REC("v");
}
#undef DS2_XL_BWD_REC

// the stacked fp16 (hi; lo) A-fragment slots of value (row m < 8, k) in a 1-KB fragment:
// lane (k >> 3) * 16 + m (hi) / + m + 8 (lo), slot k & 7
__device__ __forceinline__ int xl_frag_hi(int m, int k) { return (((k >> 3) << 4) + m) * 8 + (k & 7); }

// ---------------------------------------------------------------------------------------
// forward: gh[8 samples x 96] = h_{t-1}[8 x H] . W_hh[(r, z, n) rows of 32 units]^T.
// Wave w holds W_hh for the producers [p0, p0 + np) (k = their 32 units each): per producer and
// column tile ct = gate * 2 + unit half, the fp16 hi / lo B fragments of W_hh's rows scaled by
// 2^e(gate, unit) (the row's max over the whole K).  h (|h| < 1) takes the fixed scale 2^14.
// TRACE: the instantiation with the stamp sites (DS2_GRU_STAMPS=2); the product ones carry none
// ST: step 0 starts from the caller's state (rnn_common.h FwdState)
template <int NPW, bool TRACE, typename... S>
__global__ __launch_bounds__(LT) __attribute__((amdgpu_waves_per_eu(1, 1))) void gru_fwd_xl_kernel(
    int T, int N, int H, int D, int UBX, int BTX, const float* __restrict__ xproj,
    const float* __restrict__ w_f, const float* __restrict__ w_r, const float* __restrict__ b_f,
    const float* __restrict__ b_r, const int* __restrict__ lens, float* __restrict__ h_all,
    float* __restrict__ gates, float* __restrict__ ring, unsigned* __restrict__ xl,
    unsigned* __restrict__ err, unsigned* __restrict__ err_out,
    unsigned long long* __restrict__ stamps, int force_global, S... sp) {
  constexpr bool ST = sizeof...(S) != 0;
  const FwdState st = fwd_state(sp...);
  constexpr int NCT = 6;
  __shared__ float red[LW * 3 * 256];   // folded partials (xl_fold_at); the start-up row maxima
  __shared__ __attribute__((aligned(16))) _Float16 stg[64 * 8];
  __shared__ float unsc[3 * LU];
  __shared__ __attribute__((aligned(16))) float pin[3 * 256];    // xproj (r, z, n) [gate][sample][unit]
  __shared__ __attribute__((aligned(16))) float pout[5 * 256];   // h, r, z, n, W_hn h + b_hn
  __shared__ int slen[LB];
  __shared__ int sh_local;
  __shared__ int failed;
  __shared__ XlCold cold;
  // W_hh fragments of a wave's last producer when it has NPW + 1 (cfg2: 25 = 6 + 6 + 6 + 7):
  // in LDS, read every step, instead of 48 more registers in every wave
  __shared__ u32x4 wx[LW * NCT * 2 * 64];
  const int G = D * BTX;
  int g, ub;
  if (!xl_map(G, UBX, g, ub)) return;
  const int d = g / BTX, bt = g - d * BTX;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the wave's producers: UBX / 4 each and one more for the lowest UBX % 4 waves -- wave 0,
  // which issues none of the step's HBM traffic (the io waves below), takes the extra one
  const int p0 = wave * (UBX / LW) + min(wave, UBX % LW);
  const int np = UBX / LW + (wave < UBX % LW ? 1 : 0);   // host guarantees np <= NPW + 1
  if (threadIdx.x == 0) {
    failed = 0;
    cold = XlCold{(xl_gu32*)err, (xl_gu32*)err_out, (xl_gf32*)h_all, N, D, H, bt * LB, ub * LU};
  }
  const bool local =
      xl_group_local(xl + g * 32, ub, UBX, err, err_out, &sh_local, xl + 512 + g, force_global);
  const int slot_floats = G * UBX * 256;
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc(ring, (short)0, LSLOTS * slot_floats * 4, 0x00020000);
  const int grp_off = g * UBX * 256;
  // per-wave timeline (DS2_GRU_STAMPS=2): [step][block][wave][6] = step start, hand-off wait
  // done, products done, io done (waves 1-3), reduction barrier done, published; lane 0 of
  // every wave (scripts/trace_gru.py)
  auto trace_at = [&](int s, int p) __attribute__((always_inline)) {
    if constexpr (TRACE)
      if (stamps != nullptr && lane == 0 && s >= kXlTraceS0 && s < kXlTraceS0 + kXlTraceSteps)
        stamps[(((int64_t)(s - kXlTraceS0) * gridDim.x + blockIdx.x) * LW + wave) * 6 + p] =
            __builtin_amdgcn_s_memrealtime();
  };

  // W_hh fragments: producer p, tile ct (gate gt = ct >> 1, half c = ct & 1), k slot i ->
  // W[gt H + 32 ub + 16 c + (lane & 15)][32 (p0 + p) + 8 (lane >> 4) + i]
  // (producers below kXlVgprW in VGPRs, the others in AGPRs, producer NPW in LDS)
  u32x4 whi[NPW][NCT], wlo[NPW][NCT];
  {
    const float* W = d == 0 ? w_f : w_r;
    const int q8 = 8 * (lane >> 4);
    auto frag = [&](int p, int ct, f32x4& a, f32x4& b) __attribute__((always_inline)) {
      const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p < np) {
        const float* r = W + (int64_t)((ct >> 1) * H + LU * ub + 16 * (ct & 1) + (lane & 15)) * H +
                         LU * (p0 + p) + q8;
        a = *reinterpret_cast<const f32x4*>(r);
        b = *reinterpret_cast<const f32x4*>(r + 4);
      } else {
        a = z4;
        b = z4;
      }
    };
    float mx[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) mx[ct] = 0.f;
#pragma unroll
    for (int p = 0; p < NPW + 1; ++p)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        f32x4 a, b;
        frag(p, ct, a, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) mx[ct] = fmaxf(mx[ct], fmaxf(fabsf(a[i]), fabsf(b[i])));
      }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      mx[ct] = fmaxf(mx[ct], __shfl_xor(mx[ct], 16));
      mx[ct] = fmaxf(mx[ct], __shfl_xor(mx[ct], 32));
      if (lane < 16) red[wave * 96 + ct * 16 + lane] = mx[ct];
    }
    __syncthreads();
    float sc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      float m = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < LW; ++w4) m = fmaxf(m, red[w4 * 96 + ct * 16 + (lane & 15)]);
      sc[ct] = __builtin_ldexpf(1.f, h3_row_exp(m));
    }
    if (threadIdx.x < 3 * LU) {   // (gate, unit) = threadIdx.x = ct * 16 + column
      float m = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < LW; ++w4) m = fmaxf(m, red[w4 * 96 + threadIdx.x]);
      unsc[threadIdx.x] = __builtin_ldexpf(1.f, -(h3_row_exp(m) + 14));
    }
    __syncthreads();
    asm volatile("" ::: "memory");   // re-load W below (do not keep the max pass's loads live)
#pragma unroll
    for (int p = 0; p < NPW + 1; ++p)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        f32x4 a, b;
        frag(p, ct, a, b);
        const Duo dd = split2h(a, b, sc[ct]);
        const u32x4 dh = __builtin_bit_cast(u32x4, dd.hi), dl = __builtin_bit_cast(u32x4, dd.lo);
        if (p < NPW) {
          whi[p < NPW ? p : 0][ct] = p < kXlVgprW ? dh : xl_agpr(dh);
          wlo[p < NPW ? p : 0][ct] = p < kXlVgprW ? dl : xl_agpr(dl);
        } else {
          wx[((wave * NCT + ct) * 2 + 0) * 64 + lane] = dh;
          wx[((wave * NCT + ct) * 2 + 1) * 64 + lane] = dl;
        }
      }
  }
  const float* bh = d == 0 ? b_f : b_r;
  const int m = threadIdx.x >> 5;        // sample of the tile
  const int u = threadIdx.x & 31;        // unit of the block
  const int n = bt * LB + m;
  const int j = ub * LU + u;
  const bool owner = n < N;
  float bias_r = 0.f, bias_z = 0.f, bias_n = 0.f;
  if (owner) {
    bias_r = bh[j];
    bias_z = bh[H + j];
    bias_n = bh[2 * H + j];
  }
  if (threadIdx.x < LB) slen[threadIdx.x] = bt * LB + (int)threadIdx.x < N ? lens[bt * LB + threadIdx.x] : 0;
  __syncthreads();
  const int len = slen[m];
  const float us_r = unsc[u], us_z = unsc[LU + u], us_n = unsc[2 * LU + u];
  settle(bias_r);
  settle(bias_z);
  settle(bias_n);
  const int shi = xl_frag_hi(m, u), slo = shi + 64;   // this owner's stg slots (lo: row + 8)
  const int fold_at = xl_fold_at(lane), fold_own = xl_fold_own(m, u);
  // The step's HBM traffic (xproj in; h_all, gates out) goes through LDS, issued by waves 1-3
  // only: wave 0 publishes, and its drain before the publish would otherwise wait for those
  // loads and stores (vmcnt counts in order).  Inputs are loaded one step ahead, after the
  // wave's hand-off loop (so they never sit in front of its tile loads); outputs of step s are
  // stored during step s + 1.  io float4 q: sample q / 24, gate (q % 24) / 8, units 4 (q % 8).
  // Addresses are set up once: each io float4 has a running row pointer that one add per step
  // advances by a signed loop-invariant stride, negative in the reverse direction (per-step
  // 64-bit index arithmetic -- a 64-bit multiply is four quarter-rate instructions -- and
  // lane-divergent branches cost ~1 us of VALU latency at one wave per SIMD); masked lanes load
  // from a valid address.  load_in and store_out are therefore called once per step, in step
  // order.
  const bool io = wave != 0;
  const int q = io ? (int)threadIdx.x - 64 : 0;
  const int qm = q / 24, qg = (q % 24) >> 3, q4 = (q & 7) * 4;
  const int qn = bt * LB + qm;
  const bool qv = io && qn < N;
  const int qlen = slen[qm];
  const float* xq = xproj + ((int64_t)qn * D + d) * 3 * H + qg * H + ub * LU + q4;
  const int t_first = d == 0 ? 0 : T - 1;
  const int64_t xstep = d == 0 ? (int64_t)N * D * 3 * H : -(int64_t)N * D * 3 * H;
  const float* xp = kAblFixT ? xq : xq + t_first * ((int64_t)N * D * 3 * H);
  const f32x4 z4v = f32x4{0.f, 0.f, 0.f, 0.f};
  // the load (from a valid address when masked) and, separately, whether step st has a row:
  // the zero select happens when the value is staged -- a select right after the load would
  // make the wave wait for it there (vmcnt(0) at issue: the whole HBM latency)
  auto in_ok = [&](int st) __attribute__((always_inline)) {
    const int tt = d == 0 ? st : T - 1 - st;
    return !kAblLoads && qv && tt < qlen;
  };
  auto load_in = [&](int st) __attribute__((always_inline)) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(in_ok(st) ? xp : xproj);
    if (!kAblFixT) xp += xstep;
    return v;
  };
  // outputs: float4 idx = q + 192 k (< 320): sample idx / 40, field (idx % 40) / 8 (h, r, z,
  // n, W_hn h + b_hn), units 4 (idx % 8)
  float* ob[2];
  int64_t ostr[2];
  int osrc[2];
  bool ov[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int idx = q + 192 * k;
    const int sm = (idx / 40) & 7, f = (idx % 40) >> 3, o4 = (idx & 7) * 4, sn = bt * LB + sm;
    ov[k] = io && idx < 320 && sn < N && (f == 0 || gates != nullptr);
    osrc[k] = f * 256 + sm * LU + o4;
    if (f == 0) {
      ob[k] = h_all + ((int64_t)sn * D + d) * H + ub * LU + o4;
      ostr[k] = (int64_t)N * D * H;
    } else {
      ob[k] = gates + ((int64_t)sn * D + d) * 4 * H + (f - 1) * H + ub * LU + o4;
      ostr[k] = (int64_t)N * D * 4 * H;
    }
    ob[k] += t_first * ostr[k];
    if (d != 0) ostr[k] = -ostr[k];
  }
  // pout -> h_all, gates, the rows of step 0 at the first call and of the next step at each
  // call after it: both LDS reads, one wait, the stores
  auto store_out = [&]() __attribute__((always_inline)) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(pout + osrc[0]);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(pout + osrc[1]);
    if (ov[0]) *reinterpret_cast<f32x4*>(ob[0]) = v0;
    if (ov[1]) *reinterpret_cast<f32x4*>(ob[1]) = v1;
    ob[0] += ostr[0];
    ob[1] += ostr[1];
  };
  // one step ahead (vmcnt counts in order: a load still in flight would hold back the next
  // step's tile waits whatever its own use, so a longer prefetch distance buys nothing)
  f32x4 xin = io ? load_in(0) : z4v;
  float h_own = 0.f;
  float cin[3] = {0.f, 0.f, 0.f};   // ST: hproj0 (r, z, n), zero after step 0
  if constexpr (ST) {
    if (owner) {
#pragma unroll
      for (int gt = 0; gt < 3; ++gt) cin[gt] = st.hproj0[(int64_t)n * 3 * H + gt * H + j];
      h_own = st.h0[(int64_t)n * H + j];
    }
#pragma unroll
    for (int gt = 0; gt < 3; ++gt) settle(cin[gt]);
    settle(h_own);
  }
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? s : T - 1 - s;
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    trace_at(s, 0);
    // the step's inputs (loaded during the last step), staged before the tile loads: the wait
    // for them overlaps the producers' latency, and nothing HBM-bound is left in flight in
    // front of the tile loads
    if (io) *reinterpret_cast<f32x4*>(pin + qg * 256 + qm * LU + q4) = in_ok(s) ? xin : z4v;
    if (s > 0) {
      trace_at(s, 1);
      const int base = (((s - 1) % LSLOTS) * slot_floats + grp_off + p0 * 256 + lane * 4) * 4;
      sleep_units(g_rnn_tune[7]);
      u32x4 hv[NPW + 1];
      // the tile count as the step sees it: opaque, so that each `p < npl` is a scalar compare
      // where it is used -- with np itself the compiler hoists every one of them out of the
      // step loop as a 64-bit lane mask, and those masks were most of the SGPR spills (48 at
      // NPW 6, reloaded by v_readlane in front of every tile)
      int npl = np;
      asm volatile("" : "+s"(npl));
#pragma unroll
      for (int p = 0; p < NPW + 1; ++p)
        hv[p] = __builtin_amdgcn_raw_buffer_load_b128(x_rs, p < npl ? base + p * 1024 : 0x7ffffff0, 0, kSc1);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      // fixed order: tile p is multiplied once it and every tile before it have arrived; a
      // stale pass re-loads every tile not yet multiplied (their round trips overlap)
      // Only the waits are conditional: the MFMAs of the wave's np tiles run in one straight
      // line that is left after the last one, so each acc[ct] is a single chain in one set of
      // registers (with each tile's MFMAs under that tile's condition the compiler copied all
      // 24 accumulators at every tile boundary and drained the MFMA pipe there).
      bool bad = false;   // a tile of this wave timed out: no more waits, the step is discarded
#pragma unroll
      for (int p = 0; p < NPW + 1; ++p) {
        if (p >= npl) break;
        if (!bad) {
          for (unsigned spins = 0;
               !kAblWait && (!wave_ready(__builtin_bit_cast(f32x4, hv[p])) || g_spin_limit == 0);
               ++spins) {
            if (spins > g_spin_limit || g_spin_limit == 0) {
              if (lane == 0) xl_raise(cold);
              failed = 1;
              bad = true;
              break;
            }
            sleep_units(g_rnn_tune[0]);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int q = p; q < NPW + 1; ++q)
              if (q < npl && (unsigned)(q - p) < g_rnn_tune[6])
                hv[q] = __builtin_amdgcn_raw_buffer_load_b128(x_rs, base + q * 1024, 0, kSc1);
          }
        }
        // one chain per column tile over the producers, small products first (mma3h's order).
        // Per-producer zero-C chains joined by the VALU (the backward's form) moved the bs-32
        // step's bias gradients by 3 % and cost 0.6 us per step: the adds wait on each MFMA
        if (p < kXlVgprW && p < NPW) {
          xl_fwd_tile<false>(acc, hv[p], wlo[p < NPW ? p : 0], whi[p < NPW ? p : 0]);
        } else if (p < NPW) {
          xl_fwd_tile<true>(acc, hv[p], wlo[p < NPW ? p : 0], whi[p < NPW ? p : 0]);
        } else {
          u32x4 xh[NCT], xw[NCT];
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            xh[ct] = wx[((wave * NCT + ct) * 2 + 0) * 64 + lane];
            xw[ct] = wx[((wave * NCT + ct) * 2 + 1) * 64 + lane];
          }
          xl_fwd_tile<false>(acc, hv[p], xw, xh);
        }
      }
      xl_mfma_settle(acc);
      trace_at(s, 2);
    }
    if (io) {
      if (s + 1 < T) xin = load_in(s + 1);
      if (!kAblStores && s > 0) store_out();
    }
    trace_at(s, 3);
    // the wave's partial: acc[ct][i] is row 4 (lane >> 4) + i (0-7 hi products, 8-15 lo
    // products) of column ct * 16 + (lane & 15) = gate * 32 + unit; hi + lo folded (xl_fold)
#pragma unroll
    for (int gt = 0; gt < 3; ++gt)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        red[(wave * 3 + gt) * 256 + fold_at + 32 * i] = xl_fold(acc[2 * gt][i], acc[2 * gt + 1][i]);
    __syncthreads();
    // One batch of LDS reads.  The failure word (set, if at all, in front of the barrier above)
    // rides along and is branched on at the publish barrier: read and tested right here it was
    // an LDS round trip of its own in front of the first partial, every step.  A failed step's
    // gate math runs on whatever the tiles held; nothing of it leaves the workgroup.  The
    // partials and inputs come in the order the gate math wants them: r, whose sigmoid feeds the
    // tanh, then W_hn h, then z.
    const int fail = failed;
    float pr[3][LW];
#pragma unroll
    for (int w4 = 0; w4 < LW; ++w4) pr[0][w4] = red[(w4 * 3 + 0) * 256 + fold_own];
    const float xr = pin[m * LU + u];
#pragma unroll
    for (int w4 = 0; w4 < LW; ++w4) pr[2][w4] = red[(w4 * 3 + 2) * 256 + fold_own];
    const float xn = pin[512 + m * LU + u];
#pragma unroll
    for (int w4 = 0; w4 < LW; ++w4) pr[1][w4] = red[(w4 * 3 + 1) * 256 + fold_own];
    const float xz = pin[256 + m * LU + u];
    trace_at(s, 4);
    float gh[3];   // per gate ((((0 + p0) + p1) + p2) + p3), p = a wave's hi + lo
#pragma unroll
    for (int gt = 0; gt < 3; ++gt) {
      float v = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < LW; ++w4) v += pr[gt][w4];
      gh[gt] = v;
    }
    float hout = 0.f, r = 0.f, z = 0.f, nn = 0.f, ghn = 0.f;
    if constexpr (ST) {
      if (owner && t < len) {
        ghn = gh[2] * us_n + cin[2] + bias_n;
        r = sigmoid_fast(gh[0] * us_r + cin[0] + bias_r + xr);
        z = sigmoid_fast(gh[1] * us_z + cin[1] + bias_z + xz);
        nn = tanh_fast(xn + r * ghn);
        hout = (h_own - nn) * z + nn;
      }
#pragma unroll
      for (int gt = 0; gt < 3; ++gt) cin[gt] = 0.f;
    } else if (owner && t < len) {
      ghn = gh[2] * us_n + bias_n;
      r = sigmoid_fast(gh[0] * us_r + bias_r + xr);
      z = sigmoid_fast(gh[1] * us_z + bias_z + xz);
      nn = tanh_fast(xn + r * ghn);
      hout = (h_own - nn) * z + nn;
    }
    h_own = owner ? hout : 0.f;
    pout[m * LU + u] = hout;
    pout[256 + m * LU + u] = r;
    pout[512 + m * LU + u] = z;
    pout[768 + m * LU + u] = nn;
    pout[1024 + m * LU + u] = ghn;
    {
      const float v = hout * 16384.f;
      const _Float16 hi = (_Float16)v;
      stg[shi] = hi;
      stg[slo] = (_Float16)(v - (float)hi);
    }
    // the publish slots' offsets do not depend on the step's data: scalars, ready before the
    // barrier; the lane's part (lane * 16) is loop-invariant
    const int pub_at = ((s % LSLOTS) * slot_floats + grp_off + ub * 256) * 4;
    const int sen_at = (((s + 2) % LSLOTS) * slot_floats + grp_off + ub * 256) * 4;
    __syncthreads();
    if (fail) {   // a wave's tile timed out: poison what is left, publish nothing
      xl_poison(cold, s, T, d != 0, d, 1, 1);
      return;
    }
    if (wave == 0) {
      const u32x4 v = desentinel(*reinterpret_cast<const u32x4*>(stg + lane * 8));
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // last step's sentinel store first
      xl_store(v, x_rs, lane * 16, pub_at, local);
      xl_store(u32x4{kSentinel, kSentinel, kSentinel, kSentinel}, x_rs, lane * 16, sen_at, local);
    }
    trace_at(s, 5);
  }
  __syncthreads();
  if (io && !kAblStores) store_out();
}

// ---------------------------------------------------------------------------------------
// backward: rec[8 samples x 32 units] = dG[8 x 3H] . W_hh[3H rows, 32 units], dG = the (dar,
// daz, dghn) gate gradients of the step after.  Producer p publishes per step ONE record: per
// gate the stacked (hi; lo) fp16 A fragment of its 8 x 32 gradients, each sample row scaled by
// its own 2^e (max over the row's 96 values), then the 8 factors 2^-e.  Wave w holds W_hh^T's
// fragments for the producers [p0, p0 + np): per producer, gate and unit half, hi / lo of the
// 32 rows of that gate block in the consumer's 16 columns, each column scaled by 2^e(unit)
// (its max over the whole 3H).  Per record: 12 MFMAs from zero C, (C1 + C2) scaled per row and
// added to the wave's partial in producer order.
// Per-producer flags: the records as their own flags (the forward's sentinel ring over 3.1-KB
// records, no drain and no flag) measured 5.3-5.5 vs 3.8 us per step and was removed.
// ROWS: the instantiation that also keeps the row maxima of dgx (rowp)
template <int NPW, bool ROWS, bool TRACE>
__global__ __launch_bounds__(LT) __attribute__((amdgpu_waves_per_eu(1, 1))) void gru_bwd_xl_kernel(
    int T, int N, int H, int D, int UBX, int BTX, const float* __restrict__ dy, int dyd,
    const float* __restrict__ w_f, const float* __restrict__ w_r,
    const float* __restrict__ h_all, const float* __restrict__ gates,
    const int* __restrict__ lens, float* __restrict__ dgx, float* __restrict__ dgh,
    float* __restrict__ ring, unsigned* __restrict__ xl, unsigned* __restrict__ err,
    unsigned* __restrict__ err_out, unsigned long long* __restrict__ stamps,
    double* __restrict__ dbp, unsigned* __restrict__ camax, float* __restrict__ rowp,
    int force_global) {
  constexpr int LWP = 3;     // records in flight per wave beside the one multiplied
  __shared__ __attribute__((aligned(8))) float red[4 * LB * LU * 2];   // folded partials (xl_fold_at); the epilogue's sums
  __shared__ __attribute__((aligned(16))) _Float16 stg[3 * 64 * 8];
  __shared__ __attribute__((aligned(16))) float stsc[LB];
  __shared__ float colmx[LW * LU];
  __shared__ __attribute__((aligned(16))) float pin[6 * 256];    // dy, r, z, n, W_hn h + b_hn, h_prev
  __shared__ __attribute__((aligned(16))) float pout[4 * 256];   // dar, daz, dan, dghn
  __shared__ int slen[LB];
  __shared__ int sh_local;
  __shared__ int flag;
  __shared__ XlCold cold;
  __shared__ float rowmx[2 * LB];   // dgx row maxima of the last two steps (rowp)
  // W_hh^T fragments of a wave's last producer when it has NPW + 1 (as the forward's)
  __shared__ u32x4 wx[LW * 6 * 2 * 64];
  const int G = D * BTX;
  int g, ub;
  if (!xl_map(G, UBX, g, ub)) return;
  const int d = g / BTX, bt = g - d * BTX;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the wave's producers: UBX / 4 each and one more for the lowest UBX % 4 waves -- wave 0,
  // which issues none of the step's HBM traffic (the io waves below), takes the extra one
  const int p0 = wave * (UBX / LW) + min(wave, UBX % LW);
  const int np = UBX / LW + (wave < UBX % LW ? 1 : 0);   // host guarantees np <= NPW + 1
  const int H3 = 3 * H;
  if (threadIdx.x == 0) {
    flag = 1;
    cold = XlCold{(xl_gu32*)err, (xl_gu32*)err_out, (xl_gf32*)dgx, N, D, H, bt * LB, ub * LU};
  }
  const int slot_floats = G * UBX * LRB;
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc(ring, (short)0, 2 * slot_floats * 4, 0x00020000);
  const int grp_off = g * UBX * LRB;
  const bool local =
      xl_group_local(xl + g * 32, ub, UBX, err, err_out, &sh_local, xl + 512 + g, force_global);
  unsigned* flags = xl + 256 + g * 32;
  const __amdgpu_buffer_rsrc_t f_rs =
      __builtin_amdgcn_make_buffer_rsrc(xl + 256, (short)0, 8 * 32 * 4, 0x00020000);
  // per-wave timeline (DS2_GRU_STAMPS=2): [step][block][wave][6] = step start, hand-off wait
  // done, products done, io done (waves 1-3), reduction barrier done, published; lane 0 of
  // every wave (scripts/trace_gru.py)
  auto trace_at = [&](int s, int p) __attribute__((always_inline)) {
    if constexpr (TRACE)
      if (stamps != nullptr && lane == 0 && s >= kXlTraceS0 && s < kXlTraceS0 + kXlTraceSteps)
        stamps[(((int64_t)(s - kXlTraceS0) * gridDim.x + blockIdx.x) * LW + wave) * 6 + p] =
            __builtin_amdgcn_s_memrealtime();
  };

  // W_hh^T fragments: producer p, gate gt, half c, k slot i ->
  //   W_hh[gt H + 32 (p0 + p) + 8 (lane >> 4) + i][32 ub + 16 c + (lane & 15)]
  // [hi, lo] last; producer 0 in VGPRs, the others in AGPRs, producer NPW in LDS
  u32x4 w[NPW][3][2][2];
  float unscale;   // 2^-e of the owner's unit (threadIdx.x & 31)
  {
    const float* W = d == 0 ? w_f : w_r;
    const int q8 = 8 * (lane >> 4);
    auto col = [&](int p, int gt, int c, f32x4& a, f32x4& b) __attribute__((always_inline)) {
      if (p < np) {
        const float* wc = W + (int64_t)(gt * H + LU * (p0 + p) + q8) * H + LU * ub + 16 * c + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = wc[(int64_t)i * H];
          b[i] = wc[(int64_t)(i + 4) * H];
        }
      } else {
        a = f32x4{0.f, 0.f, 0.f, 0.f};
        b = a;
      }
    };
    float mx[2] = {0.f, 0.f};
#pragma unroll
    for (int p = 0; p < NPW + 1; ++p)
#pragma unroll
      for (int gt = 0; gt < 3; ++gt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          f32x4 a, b;
          col(p, gt, c, a, b);
#pragma unroll
          for (int i = 0; i < 4; ++i) mx[c] = fmaxf(mx[c], fmaxf(fabsf(a[i]), fabsf(b[i])));
        }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], 16));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], 32));
      if (lane < 16) colmx[wave * LU + 16 * c + lane] = mx[c];
    }
    __syncthreads();
    float sc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float m = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < LW; ++w4) m = fmaxf(m, colmx[w4 * LU + 16 * c + (lane & 15)]);
      sc[c] = __builtin_ldexpf(1.f, h3_row_exp(m));
    }
    {
      float m = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < LW; ++w4) m = fmaxf(m, colmx[w4 * LU + (threadIdx.x & 31)]);
      unscale = __builtin_ldexpf(1.f, -h3_row_exp(m));
    }
    asm volatile("" ::: "memory");   // re-load W below (do not keep the max pass's loads live)
#pragma unroll
    for (int p = 0; p < NPW + 1; ++p)
#pragma unroll
      for (int gt = 0; gt < 3; ++gt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          f32x4 a, b;
          col(p, gt, c, a, b);
          const Duo dd = split2h(a, b, sc[c]);
          const u32x4 dh = __builtin_bit_cast(u32x4, dd.hi), dl = __builtin_bit_cast(u32x4, dd.lo);
          if (p < NPW) {
            w[p < NPW ? p : 0][gt][c][0] = p < kXlVgprWBwd ? dh : xl_agpr(dh);
            w[p < NPW ? p : 0][gt][c][1] = p < kXlVgprWBwd ? dl : xl_agpr(dl);
          } else {
            wx[((wave * 6 + gt * 2 + c) * 2 + 0) * 64 + lane] = dh;
            wx[((wave * 6 + gt * 2 + c) * 2 + 1) * 64 + lane] = dl;
          }
        }
  }
  const int m = threadIdx.x >> 5;
  const int u = threadIdx.x & 31;
  const int n = bt * LB + m;
  const bool owner = n < N;
  if (threadIdx.x < LB) slen[threadIdx.x] = bt * LB + (int)threadIdx.x < N ? lens[bt * LB + threadIdx.x] : 0;
  __syncthreads();
  const int len = slen[m];
  const int shi = xl_frag_hi(m, u), slo = shi + 64;
  const int fold_at = xl_fold_at(lane), fold_own = xl_fold_own(m, u);
  // The step's HBM traffic through LDS, issued by waves 1-3 only (as in the forward): wave 0
  // publishes, and its drain may not queue behind HBM loads or stores (vmcnt counts in order).
  // Every wave polls the flags of its own producers; an io wave's poll comes after it staged
  // the inputs it loaded a step earlier, so nothing of its own is in flight in front of it.  Inputs one step ahead, loaded after the wave's
  // record loop; the gradients of step s stored during step s + 1.  io float4 idx = q + 192 k:
  // sample idx / 48, field (idx % 48) / 8, units 4 (idx % 8).
  // Addresses set up once (as the forward's): a fixed row pointer per io float4, advanced by
  // a fixed stride per step; masked lanes load from a valid address.
  const bool io = wave != 0;
  const int q = io ? (int)threadIdx.x - 64 : 0;
  // (32-bit element offsets: the host bounds every tensor below 2^31 bytes)
  const f32x4 z4v = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ostr = N * D * H3;
  // per io float4 k (two per thread): field, sample length (-1: none), element offset of the
  // t = 0 row, stride per t, and the output offset (-1: none)
  struct IoSlot {
    const float* in;   // the input row of t = 0 (h_prev: its own t)
    float* out;        // the output row of t = 0 (nullptr: none)
    int f, len, str, pin_at, pout_at;
  };
  auto make_slot = [&](int k) __attribute__((always_inline)) {
    const int idx = q + 192 * k;
    const int sm = idx / 48, f = (idx % 48) >> 3, o4 = (idx & 7) * 4, sn = bt * LB + sm;
    IoSlot r;
    r.f = f;
    r.len = io && sn < N ? slen[sm] : -1;
    if (f == 0) {
      r.in = dy + (sn * dyd + (dyd > 1 ? d : 0)) * H + ub * LU + o4;
      r.str = N * dyd * H;
    } else if (f < 5) {
      r.in = gates + (sn * D + d) * 4 * H + (f - 1) * H + ub * LU + o4;
      r.str = N * D * 4 * H;
    } else {
      r.in = h_all + (sn * D + d) * H + ub * LU + o4;
      r.str = N * D * H;
    }
    r.out = io && sn < N ? (f < 3 ? dgx : dgh) + (sn * D + d) * H3 + (f % 3) * H + ub * LU + o4
                         : nullptr;
    r.pin_at = f * 256 + sm * LU + o4;
    r.pout_at = (f < 3 ? f : (f == 5 ? 3 : f - 3)) * 256 + sm * LU + o4;
    return r;
  };
  const IoSlot sl0 = make_slot(0), sl1 = make_slot(1);
  // the load, and separately whether step st has that row (the zero select is applied when the
  // value is staged: a select right after the load would wait for it there, as the forward's)
  auto in_ok = [&](int st, const IoSlot sl) __attribute__((always_inline)) {
    const int tt = d == 0 ? T - 1 - st : st;
    const int tr = sl.f == 5 ? (d == 0 ? tt - 1 : tt + 1) : tt;
    return !kAblLoads && tt < sl.len && tr >= 0 && tr < T;
  };
  auto load_in = [&](int st, const IoSlot sl) __attribute__((always_inline)) {
    const int tt = d == 0 ? T - 1 - st : st;
    const int tr = sl.f == 5 ? (d == 0 ? tt - 1 : tt + 1) : tt;
    return *reinterpret_cast<const f32x4*>(sl.in + (in_ok(st, sl) && !kAblFixT ? tr * sl.str : 0));
  };
  auto stage_in = [&](const f32x4 v, const IoSlot sl, int st) __attribute__((always_inline)) {
    *reinterpret_cast<f32x4*>(pin + sl.pin_at) = in_ok(st, sl) ? v : z4v;
  };
  auto store_one = [&](int tt, const IoSlot sl) __attribute__((always_inline)) {
    if (sl.out != nullptr)
      *reinterpret_cast<f32x4*>(sl.out + tt * ostr) = *reinterpret_cast<const f32x4*>(pout + sl.pout_at);
  };
  // pout (step st) -> dgx (dar, daz, dan), dgh (dar, daz, dghn)
  auto store_out = [&](int st) __attribute__((always_inline)) {
    const int tt = d == 0 ? T - 1 - st : st;
    store_one(tt, sl0);
    store_one(tt, sl1);
  };
  // rowp [T N][D][UBX]: the workgroup's max |dgx| per sample row of every step (the dX GEMM's
  // row scales without a pass over dgx).  Reduced and parked in rowmx after the publish, in
  // the slack before the next step's wait; stored two steps later by the first 8 lanes of
  // wave 1 beside store_out (the reduction barrier of the step in between orders the two).
  // (32-bit element offsets, as the other outputs: rowp is smaller than dgx)
  const int rpo = ROWS && wave == 1 && lane < LB && bt * LB + lane < N
                      ? ((bt * LB + lane) * D + d) * UBX + ub
                      : -1;
  const int rpstr = N * D * UBX;
  auto store_rmx = [&](int st) __attribute__((always_inline)) {
    if (!ROWS || wave != 1) return;
    const int tt = d == 0 ? T - 1 - st : st;
    if (rpo >= 0) rowp[rpo + tt * rpstr] = rowmx[(st & 1) * LB + lane];
  };
  // one step ahead (as the forward's)
  f32x4 xin0 = io ? load_in(0, sl0) : z4v, xin1 = io ? load_in(0, sl1) : z4v;
  float dh_prev = 0.f, z_prev = 0.f;
  double sb_r = 0.0, sb_z = 0.0, sb_n = 0.0, sb_hn = 0.0;
  float cm_r = 0.f, cm_z = 0.f, cm_n = 0.f, cm_hn = 0.f;
  const int rsel = ((lane >> 4) & 1) * 16;   // this lane's 4 row factors (samples 4 (..) + i)
  // the io waves' issue point: right after a step's last record load (the records are then
  // older than these loads and stores, so the record waits never queue behind HBM: vmcnt
  // counts in order), inputs for the next step and the outputs of the previous one
  auto io_issue = [&](int st) __attribute__((always_inline)) {
    if (!io) return;
    if (st + 1 < T) {
      xin0 = load_in(st + 1, sl0);
      xin1 = load_in(st + 1, sl1);
    }
    if (!kAblStores && st > 0) store_out(st - 1);
    if (!kAblStores && st > 1) store_rmx(st - 2);
  };
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? T - 1 - s : s;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    trace_at(s, 0);
    if (io) {   // the step's inputs (loaded during the last step), before the wave's poll
      stage_in(xin0, sl0, s);
      stage_in(xin1, sl1, s);
    }
    if (s == 0) io_issue(0);
    if (s > 0) {
      int npl = np;   // opaque per step (as the forward's): scalar compares, no hoisted lane masks
      asm volatile("" : "+s"(npl));
      // a wave whose wait timed out clears `flag`; the workgroup leaves at the reduction barrier
      if (!kAblWait && !xl_wave_flags_wait(flags + p0, npl, (unsigned)s, cold) && lane == 0)
        flag = 0;
      asm volatile("" ::: "memory");
      trace_at(s, 1);
      const int rb = (((s - 1) & 1) * slot_floats + grp_off + p0 * LRB) * 4;
      u32x4 r0[NPW + 1], r1[NPW + 1], r2[NPW + 1];
      f32x4 rs[NPW + 1];
      auto load_rec = [&](int p) __attribute__((always_inline)) {
        const int base = p < npl ? rb + p * LRB * 4 : 0x7ffff000;
        r0[p] = __builtin_amdgcn_raw_buffer_load_b128(x_rs, base + lane * 16, 0, kSc1);
        r1[p] = __builtin_amdgcn_raw_buffer_load_b128(x_rs, base + 1024 + lane * 16, 0, kSc1);
        r2[p] = __builtin_amdgcn_raw_buffer_load_b128(x_rs, base + 2048 + lane * 16, 0, kSc1);
        rs[p] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, base + 3072 + rsel, 0, kSc1));
      };
#pragma unroll
      for (int p = 0; p < LWP && p < NPW + 1; ++p) load_rec(p);
      if (LWP >= NPW + 1) io_issue(s);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < NPW + 1; ++p) {
        if (p + LWP < NPW + 1) load_rec(p + LWP);
        if (p + LWP == NPW) io_issue(s);
        if (p < npl) {
          f32x4 cc[4];
          if (p < kXlVgprWBwd && p < NPW) {
            xl_bwd_rec<false>(cc, r0[p], r1[p], r2[p], w[p < NPW ? p : 0]);
          } else if (p < NPW) {
            xl_bwd_rec<true>(cc, r0[p], r1[p], r2[p], w[p < NPW ? p : 0]);
          } else {
            u32x4 xw[3][2][2];
#pragma unroll
            for (int k = 0; k < 12; ++k)
              xw[k >> 2][(k >> 1) & 1][k & 1] = wx[(wave * 12 + k) * 64 + lane];
            xl_bwd_rec<false>(cc, r0[p], r1[p], r2[p], xw);
          }
          // (c1 + c2) 2^-e per sample row, in producer order
          acc[0] += (cc[0] + cc[1]) * rs[p];
          acc[1] += (cc[2] + cc[3]) * rs[p];
        }
      }
      trace_at(s, 2);
    }
    trace_at(s, 3);
    // acc[c][i]: row 4 (lane >> 4) + i of unit 16 c + (lane & 15); hi + lo folded (xl_fold)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave * 256 + fold_at + 32 * i] = xl_fold(acc[0][i], acc[1][i]);
    __syncthreads();
    // one batch of LDS reads; the flag word (cleared, if at all, in front of the barrier above)
    // rides along and is branched on at the publish barrier, as the forward's failure word
    const int flag_v = flag;
    float pr[LW];
#pragma unroll
    for (int w4 = 0; w4 < LW; ++w4) pr[w4] = red[w4 * 256 + fold_own];
    const float dyv = pin[m * LU + u], g_r = pin[256 + m * LU + u], g_z = pin[512 + m * LU + u];
    const float g_n = pin[768 + m * LU + u], g_hn = pin[1024 + m * LU + u];
    const float hp = pin[1280 + m * LU + u];
    trace_at(s, 4);
    float dar = 0.f, daz = 0.f, dan = 0.f, dghn = 0.f;
    if (owner) {
      float dh = 0.f, zc = 0.f;
      if (t < len) {
        float carry = 0.f;
        if (s > 0) {
          float rec = 0.f;   // (((0 + p0) + p1) + p2) + p3, p = a wave's hi + lo
#pragma unroll
          for (int w4 = 0; w4 < LW; ++w4) rec += pr[w4];
          carry = dh_prev * z_prev + rec * unscale;
        }
        dh = dyv + carry;
        zc = g_z;
        // (1 - n^2 as one fma, written out: left to the compiler's contraction the choice
        // between it and a multiply + subtract follows the surrounding code, and the bits with it)
        dan = dh * (1.f - zc) * __builtin_fmaf(-g_n, g_n, 1.f);
        daz = dh * (hp - g_n) * zc * (1.f - zc);
        dar = dan * g_hn * g_r * (1.f - g_r);
        dghn = dan * g_r;
      }
      dh_prev = dh;
      z_prev = zc;
    }
    {
      // the row's scale: max over the sample's 32 units x 3 gates (32 consecutive lanes)
      const float mx = half_wave_max(fmaxf(fmaxf(fabsf(dar), fabsf(daz)), fabsf(dghn)));
      const int e = h3_row_exp(mx);
      const float sc = __builtin_ldexpf(1.f, e);
      const float vr = dar * sc, vz = daz * sc, vn = dghn * sc;
      const _Float16 hr = (_Float16)vr, hz = (_Float16)vz, hn = (_Float16)vn;
      stg[shi] = hr;
      stg[slo] = (_Float16)(vr - (float)hr);
      stg[512 + shi] = hz;
      stg[512 + slo] = (_Float16)(vz - (float)hz);
      stg[1024 + shi] = hn;
      stg[1024 + slo] = (_Float16)(vn - (float)hn);
      if (u == 0) stsc[m] = __builtin_ldexpf(1.f, -e);
    }
    // (the record's fragments first: dgx / dgh are only stored during the next step)
    pout[m * LU + u] = dar;
    pout[256 + m * LU + u] = daz;
    pout[512 + m * LU + u] = dan;
    pout[768 + m * LU + u] = dghn;
    // What neither the record nor its flag needs -- the fp64 bias-gradient sums, the column
    // maxima, the ROWS row maximum -- runs behind the publish barrier: on wave 0 between the
    // record's stores and their drain, in the shadow of that round trip.
    auto off_chain = [&]() __attribute__((always_inline)) {
      if (owner) {
        sb_r += dar; sb_z += daz; sb_n += dan; sb_hn += dghn;
        cm_r = fmaxf(cm_r, fabsf(dar));
        cm_z = fmaxf(cm_z, fabsf(daz));
        cm_n = fmaxf(cm_n, fabsf(dan));
        cm_hn = fmaxf(cm_hn, fabsf(dghn));
      }
      if (ROWS) {
        // max over the sample's 32 units x 3 gates of dgx (32 consecutive lanes); 0 where t >= len
        const float rm = half_wave_max(fmaxf(fmaxf(fabsf(dar), fabsf(daz)), fabsf(dan)));
        if (u == 0) rowmx[(s & 1) * LB + m] = rm;
      }
    };
    const int so = ((s & 1) * slot_floats + grp_off + ub * LRB) * 4;   // scalar, before the barrier
    __syncthreads();
    if (flag_v == 0) {   // a wave's flag wait timed out: poison what is left, publish nothing
      xl_poison(cold, s, T, d == 0, d, 3, 3);
      return;
    }
    if (wave == 0) {
      // the record out of LDS in one batch, then its stores under one test of `local` (a test
      // per store made each of the four an LDS round trip of its own: read, wait, store)
      u32x4 rv[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) rv[k] = *reinterpret_cast<const u32x4*>(stg + k * 512 + lane * 8);
      const u32x4 sv = *reinterpret_cast<const u32x4*>(stsc + (lane & 1) * 4);
      if (local) {
#pragma unroll
        for (int k = 0; k < 3; ++k) xl_store(rv[k], x_rs, lane * 16, so + k * 1024, true);
        if (lane < 2) xl_store(sv, x_rs, lane * 16, so + 3072, true);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) xl_store(rv[k], x_rs, lane * 16, so + k * 1024, false);
        if (lane < 2) xl_store(sv, x_rs, lane * 16, so + 3072, false);
      }
    } else {
      trace_at(s, 5);
    }
    off_chain();
    if (wave == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) {
        const unsigned fv = (unsigned)s + 1;
        if (local)
          __builtin_amdgcn_raw_buffer_store_b32(fv, f_rs, (g * 32 + ub) * 4, 0, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b32(fv, f_rs, (g * 32 + ub) * 4, 0, kSc1);
      }
      trace_at(s, 5);
    }
  }
  __syncthreads();
  if (io && !kAblStores) store_out(T - 1);
  if (!kAblStores) {
    if (T > 1) store_rmx(T - 2);
    store_rmx(T - 1);
  }
  if (camax != nullptr) {
    // column maxima of dgx [T N][D 3H] into camax[0, D 3H) and dgh into [D 3H, 2 D 3H): the 8
    // samples' running maxima per unit, one unsigned atomic max per (gate, unit)
    __syncthreads();
    red[(0 * LB + m) * LU + u] = cm_r;
    red[(1 * LB + m) * LU + u] = cm_z;
    red[(2 * LB + m) * LU + u] = cm_n;
    red[(3 * LB + m) * LU + u] = cm_hn;
    __syncthreads();
    if (threadIdx.x < 4 * LU) {
      const int gq = threadIdx.x / LU, uu = threadIdx.x - gq * LU;
      float a = 0.f;
#pragma unroll
      for (int mm = 0; mm < LB; ++mm) a = fmaxf(a, red[(gq * LB + mm) * LU + uu]);
      const unsigned bits = __float_as_uint(a);
      const int cl = d * H3 + ub * LU + uu;
      if (bits != 0u) {
        if (gq < 2) {
          atomicMax(camax + cl + gq * H, bits);
          atomicMax(camax + D * H3 + cl + gq * H, bits);
        } else if (gq == 2) {
          atomicMax(camax + cl + 2 * H, bits);
        } else {
          atomicMax(camax + D * H3 + cl + 2 * H, bits);
        }
      }
    }
  }
  if (dbp == nullptr) return;
  // the workgroup's 8 samples summed per unit in sample order -> dbp[bt][d][4][H]
  double* rd = reinterpret_cast<double*>(red);
  __syncthreads();
  rd[(0 * LB + m) * LU + u] = owner ? sb_r : 0.0;
  rd[(1 * LB + m) * LU + u] = owner ? sb_z : 0.0;
  rd[(2 * LB + m) * LU + u] = owner ? sb_n : 0.0;
  rd[(3 * LB + m) * LU + u] = owner ? sb_hn : 0.0;
  __syncthreads();
  if (threadIdx.x < 4 * LU) {
    const int gq = threadIdx.x / LU, uu = threadIdx.x - gq * LU;
    double a = 0.0;
#pragma unroll
    for (int mm = 0; mm < LB; ++mm) a += rd[(gq * LB + mm) * LU + uu];
    dbp[(((int64_t)bt * D + d) * 4 + gq) * H + ub * LU + uu] = a;
  }
}

// ---------------------------------------------------------------------------------------
// One preparation launch per recurrence call instead of two fills: zeroes `za` / `zb` (the
// counter area; the backward's column maxima) and sets every word of `ff` (the part of the
// forward's sentinel ring these kernels use) to the sentinel.  ff is 16-B aligned, ff16 its
// length in 16-B units.
__global__ __launch_bounds__(256) void gru_xl_prep_kernel(unsigned* __restrict__ za, size_t na,
                                                          unsigned* __restrict__ zb, size_t nb,
                                                          u32x4* __restrict__ ff, size_t ff16) {
  const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = i0; i < na; i += step) za[i] = 0u;
  for (size_t i = i0; i < nb; i += step) zb[i] = 0u;
  for (size_t i = i0; i < ff16; i += step) ff[i] = u32x4{kSentinel, kSentinel, kSentinel, kSentinel};
}

// out[row] = max over the row's D x UBX partials the backward stored in rowp (float bits; all
// are >= 0, so the float max is the maximum of the bits): 8 lanes per row
__global__ __launch_bounds__(256) void gru_xl_row_amax_kernel(const float* __restrict__ rowp,
                                                              int rows, int parts,
                                                              unsigned* __restrict__ out) {
  const int r = (blockIdx.x * 256 + (int)threadIdx.x) >> 3, k = threadIdx.x & 7;
  float m = 0.f;
  if (r < rows)
    for (int i = k; i < parts; i += 8) m = fmaxf(m, rowp[(int64_t)r * parts + i]);
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (r < rows && k == 0) out[r] = __float_as_uint(m);
}

// ---------------------------------------------------------------------------------------
// host side (rnn_host.h; called by ds2_gru_fwd / ds2_gru_bwd in gru.hip with their workspace
// carve-up)

// DS2_GRU_XL=0 keeps the 16-unit kernels of gru_split.hip; the XCD-local kernels are fp16x3,
// so DS2_GRU_X6=0 (fp32 MFMA) and DS2_GRU_H3[_BWD]=0 (bf16x6) select the others as before.
// DS2_GRU_XL=2 (test) runs every group GLOBAL (sc1 stores), whatever the placement.
static inline bool xl_enabled() { return !env_off("DS2_GRU_XL") && !env_off("DS2_GRU_X6"); }
static inline int xl_force_global() { return env_digit("DS2_GRU_XL") == 2 ? 1 : 0; }

// the shapes the XCD-local kernels take: H a multiple of 32 with a group (H / 32 workgroups)
// inside one XCD's 32 CUs, at most 8 groups (D x ceil(N / 8)), W_hh fragments within the
// instantiated producers per wave
int gru_xl_groups(int n, int h, int num_dirs) {
  if (!xl_enabled() || n < 1 || h < LU || (h % LU) != 0) return 0;
  const int UBX = h / LU, BTX = (n + LB - 1) / LB, G = num_dirs * BTX;
  if (UBX > 32 || G > 8 || (UBX + LW - 1) / LW > 7) return 0;
  return G;
}

// workgroups the launch holds (the blocks of unused groups return at once)
int gru_xl_active(int n, int h, int num_dirs) {
  const int G = gru_xl_groups(n, h, num_dirs);
  return G > 0 ? G * (h / LU) : 0;
}

// counter words the kernels use after the error word: 8 x 32 XCC ids, 8 x 32 flags, 8 mode words
size_t gru_xl_ctr_words() { return 520; }

// K = producers per wave: K - 1 in registers + one from LDS
// [1]: the traced instantiations, run when the caller asked for stamps (DS2_GRU_STAMPS=2)
#define DS2_XL_TABLE(K, ...) \
  {inst(2, K<1, __VA_ARGS__>), inst(4, K<3, __VA_ARGS__>), inst(7, K<6, __VA_ARGS__>)}
static const Instance kFwdXl[2][3] = {DS2_XL_TABLE(gru_fwd_xl_kernel, false),
                                      DS2_XL_TABLE(gru_fwd_xl_kernel, true)};
// with an initial state (ds2_gru_fwd_state), same keys
static const Instance kFwdXlSt[2][3] = {DS2_XL_TABLE(gru_fwd_xl_kernel, false, FwdState),
                                        DS2_XL_TABLE(gru_fwd_xl_kernel, true, FwdState)};
static const Instance kBwdXl[2][3] = {DS2_XL_TABLE(gru_bwd_xl_kernel, false, false),
                                      DS2_XL_TABLE(gru_bwd_xl_kernel, false, true)};
// the same with the row-maximum partials of dgates_x
static const Instance kBwdXlRows[2][3] = {DS2_XL_TABLE(gru_bwd_xl_kernel, true, false),
                                          DS2_XL_TABLE(gru_bwd_xl_kernel, true, true)};
#undef DS2_XL_TABLE

// ring bytes: forward 4 slots of 1-KB tiles, backward 2 slots of records (both within the
// rings ds2_gru_fwd / ds2_gru_bwd carve for the 16-unit kernels)
size_t gru_xl_ring_bytes(int n, int h, int num_dirs, bool bwd) {
  const size_t UBX = h / LU, G = (size_t)num_dirs * ((n + LB - 1) / LB);
  return bwd ? 2 * G * UBX * LRB * sizeof(float) : LSLOTS * G * UBX * 256 * sizeof(float);
}

// The one preparation launch (gru_xl_prep_kernel): zeroes the counter area [ctrs, + ctr_bytes)
// and `zb` (nb words, nullable), fills ff_bytes of the ring with the sentinel.
static bool xl_prepare(unsigned* ctrs, size_t ctr_bytes, unsigned* zb, size_t nb, float* ring,
                       size_t ff_bytes, hipStream_t st) {
  const size_t na = ctr_bytes / sizeof(unsigned), ff16 = ff_bytes / 16;
  const size_t most = std::max(std::max(na, nb), ff16);
  const unsigned grid = (unsigned)std::min<size_t>(1024, std::max<size_t>(1, (most + 255) / 256));
  hipLaunchKernelGGL(gru_xl_prep_kernel, dim3(grid), dim3(256), 0, st, ctrs, na, zb, nb,
                     reinterpret_cast<u32x4*>(ring), ff16);
  return hipGetLastError() == hipSuccess;
}

// The counter area [ho.ctrs, + ho.ctr_bytes) holds ho.err (the error word of the 16-unit
// launch over the same batch) and, right behind it, these kernels' own words.  The launches
// zero the area and set the ring's sentinels themselves, so the caller fills nothing when
// they answer true; on false the caller prepares the area for the kernel it falls back to.
// ho.err_out (nullable): the caller's status word, OR-ed by the kernel itself (no fold launch).
bool launch_gru_fwd_xl(RnnShape s, RecFwd a, Handoff ho, hipStream_t st) {
  if (gru_xl_groups(s.n, s.h, s.d) == 0 || env_off("DS2_GRU_H3")) return false;
  apply_spin_limit_env();
  apply_rnn_tune_env();
  int UBX = s.h / LU, BTX = s.BT(LB), FG = xl_force_global();
  const Instance fn = pick_instance((a.stateful() ? kFwdXlSt : kFwdXl)[ho.stamps != nullptr],
                                    (UBX + LW - 1) / LW);
  if (fn.fn == nullptr) return false;
  FwdState fs = a.state();   // the last argument, empty in the stateless instantiations
  if (!xl_prepare(ho.ctrs, ho.ctr_bytes, nullptr, 0, ho.ring,
                  gru_xl_ring_bytes(s.n, s.h, s.d, false), st))
    return false;
  unsigned* xl = ho.err + 1;
  void* args[] = {&s.t, &s.n, &s.h, &s.d, &UBX, &BTX, &a.xproj, &a.w_hh_f, &a.w_hh_r, &a.b_hh_f,
                  &a.b_hh_r, &a.lens, &a.h_all, &a.gates, &ho.ring, &xl, &ho.err, &ho.err_out,
                  &ho.stamps, &FG, &fs};
  return launch_rec(fn.fn, Ran{DS2_RUNG_XCD_LOCAL, fn.k, 0, 0, 1}, dim3(8 * UBX), dim3(LT), args,
                    ho.lds_pad, st);
}

// a.dbp: [ceil(n / 8)][D][4][H] partials (nullable); a.camax as launch_bwd16's, but zeroed by
// the preparation launch; a.rowp: [T N][D][h / 32] row-maximum partials of dgates_x (nullable)
bool launch_gru_bwd_xl(RnnShape s, RecBwd a, Handoff ho, hipStream_t st) {
  if (gru_xl_groups(s.n, s.h, s.d) == 0 || env_off("DS2_GRU_H3_BWD")) return false;
  apply_spin_limit_env();
  apply_rnn_tune_env();
  int UBX = s.h / LU, BTX = s.BT(LB), FG = xl_force_global();
  const int need = (UBX + LW - 1) / LW;
  const int tr = ho.stamps != nullptr;
  const Instance fn =
      a.rowp != nullptr ? pick_instance(kBwdXlRows[tr], need) : pick_instance(kBwdXl[tr], need);
  if (fn.fn == nullptr) return false;
  if (!xl_prepare(ho.ctrs, ho.ctr_bytes, a.camax,
                  a.camax != nullptr ? (size_t)2 * s.d * 3 * s.h : 0, nullptr, 0, st))
    return false;
  unsigned* xl = ho.err + 1;
  void* args[] = {&s.t, &s.n, &s.h, &s.d, &UBX, &BTX, &a.dy, &a.dy_dirs, &a.w_hh_f, &a.w_hh_r,
                  &a.state, &a.gates, &a.lens, &a.dgx, &a.dgh, &ho.ring, &xl, &ho.err,
                  &ho.err_out, &ho.stamps, &a.dbp, &a.camax, &a.rowp, &FG};
  return launch_rec(fn.fn, Ran{DS2_RUNG_XCD_LOCAL, fn.k, 0, 0, 1}, dim3(8 * UBX), dim3(LT), args,
                    ho.lds_pad, st);
}

// the row-maximum partials of launch_gru_bwd_xl: bytes, and their reduction to out[t_max n]
size_t gru_xl_rowp_bytes(int t_max, int n, int h, int num_dirs) {
  return (size_t)t_max * n * num_dirs * (h / LU) * sizeof(float);
}

void launch_gru_xl_row_amax(int t_max, int n, int h, int num_dirs, const float* rowp,
                            unsigned* out, hipStream_t st) {
  const int rows = t_max * n;
  hipLaunchKernelGGL(gru_xl_row_amax_kernel, dim3((rows * 8 + 255) / 256), dim3(256), 0, st, rowp,
                     rows, num_dirs * (h / LU), out);
}

}  // namespace ds2
