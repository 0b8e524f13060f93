/*
 * libds2hip — MI355X-native (gfx950 / CDNA4) DeepSpeech2 hot path, C ABI.
 *
 * The reference (vadimkantorov/deepspeech.pytorch) has no C ABI of its own: its
 * pluggable seams are Python objects whose kernels come from third-party
 * libraries (librosa FFT, cuDNN conv/BN/RNN, cuBLAS, warp-ctc, ATen argmax).
 * Every entry point below replaces one of those implicit kernels; the comment
 * above each names the reference call site (file:line) it stands in for.
 *
 * Conventions:
 *   - every function returns ds2_status_t; no exception crosses the ABI;
 *   - all buffers are caller-owned device pointers (fp32 unless noted, int32
 *     for lengths/labels), dense row-major unless a leading dimension is given;
 *   - work is enqueued on `stream` (a hipStream_t, NULL = legacy default);
 *     nothing synchronises the device, allocates, or touches host memory;
 *   - scratch memory comes in through (ws, ws_bytes); query the size with the
 *     matching *_workspace_size() function.
 */
#ifndef DS2HIP_H
#define DS2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ds2_status_t {
  DS2_OK = 0,
  DS2_INVALID_VALUE = 1,
  DS2_UNSUPPORTED_SHAPE = 2,
  DS2_HIP_ERROR = 3,
  DS2_RCCL_ERROR = 4,
  DS2_WORKSPACE_TOO_SMALL = 5
} ds2_status_t;

typedef void* ds2_stream_t; /* hipStream_t */

const char* ds2_status_string(ds2_status_t status);
const char* ds2_last_error(void);  /* text of the last HIP error seen (thread-local) */
const char* ds2_version(void);

/* ------------------------------------------------------------------------ */
/* Features: SpectrogramParser.audio_to_stft + normalize_audio('max_frame') */
/* ref data/data_loader.py:201-220,276-284; data/data_loader_aug.py:220-249,297-307 */
/* pcm:  [batch][max_samples] float32, utterance b has n_samples[b] valid samples   */
/* out:  [batch][161][max_frames], frames t >= 1 + (n_samples[b] + 2*(n_fft/2) - n_fft)/hop */
/*       (librosa's count with center=True; one fewer than 1 + n/hop when n_fft is odd and */
/*       hop divides n) are zero, and so is the whole row when n_samples[b] <= 0: the     */
/*       reference always returns 161 rows (data_loader_aug.py:234-249): the first   */
/*       161 bins when n_fft/2+1 >= 161, else its mirror-fill of ndarray.resize on    */
/*       librosa's (Fortran-ordered) stft matrix -- see stft.hip remap_kernel.         */
/* window: n_fft doubles (symmetric Hamming in the reference).                     */
/* normalize (normalize_audio, data_loader_aug.py:274-313): 0 = 'none' log1p(|X|),        */
/*   1 = 'max_frame' log1p(|X|*2^20) - mean_t(gauss20(mean_f)), 2 = 'mean' log1p(|X|) - mean, */
/*   3 = 'norm' (log1p(|X|) - mean) / mean_t(std_f), 4 = 'frame' log1p(|X|) -               */
/*   mean_t(gauss50(mean_f)); gauss_taps (2 radius + 1 scipy correlation weights) for 1, 4.  */
size_t ds2_stft_workspace_size(int batch, int max_frames, int n_fft);
ds2_status_t ds2_stft_logmag(const float* pcm, const int* n_samples, int batch, int max_samples,
                             int n_fft, int hop, const double* window, int normalize,
                             const float* gauss_taps, int gauss_radius,
                             float* out, int max_frames, void* ws, size_t ws_bytes,
                             ds2_stream_t stream);
/* The same with the spectrogram augmentations of data/data_loader_aug.py:236-248
 * (FrequencyMask / TimeMask via SOneOf, data/spectrogram_aug.py:64-117, and the
 * aug_prob_8khz cut) applied to |X| before the log, as the reference does.  masks: NULL
 * or [batch][9] int32 = {f_lo0, f_hi0, f_lo1, f_hi1, t_lo0, t_hi0, t_lo1, t_hi1, f_cut}:
 * bins in [f_lo, f_hi), frames in [t_lo, t_hi) and bins >= f_cut are zeroed (empty when
 * lo >= hi; f_cut = 161 for none), rows of the 161-row output.  The random draws stay on the host
 * (ds2amd/spect_aug.py) so they follow the reference's `random` call sequence. */
ds2_status_t ds2_stft_logmag_masked(const float* pcm, const int* n_samples, int batch,
                                    int max_samples, int n_fft, int hop, const double* window,
                                    int normalize, const float* gauss_taps, int gauss_radius,
                                    const int* masks, float* out, int max_frames, void* ws,
                                    size_t ws_bytes, ds2_stream_t stream);

/* The same frames over a stream (csrc/stft_stream.hip): PCM arrives in chunks, all n streams
 * in lock-step, and a feed returns the frames that have become final -- with a samples
 * arrived and the utterance open, frame t is final iff max(t hop - pad + n_fft - 1,
 * pad - t hop) <= a - 1 (pad = n_fft / 2: its right edge and the sample its left reflection
 * reads), which holds for the first (a >= pad + 1 ? 1 + (a + pad - n_fft) / hop : 0) frames;
 * the last feed emits the rest, up to the count above, reflecting at the true end.  A frame
 * is computed by the code ds2_stft_logmag runs, from the same samples: normalize 0 gives
 * log1p(|X|) bit for bit the rows of ds2_stft_logmag(normalize = 0) on the whole utterance,
 * over any partition.  normalize 1 gives val = log1p(|X| 2^20) minus an offset that can be
 * had on a stream (the reference's mean_t(gauss20(mean_f)) reads the whole utterance):
 *   fixed_offset != NULL   out = val - fixed_offset[b]
 *   fixed_offset == NULL   out = val - (float)off_t, off_t = (w o0 + S_t) / (w + t + 1) in
 *               fp64, S_t = S_{t-1} + (double)m_t summed in frame order, m_t the frame's
 *               float32 mean over its 161 values as ds2_stft_logmag computes it, (o0, w) the
 *               prior given to init: a pure function of the prefix, so bit for bit the same
 *               over any partition
 * Only n_fft with 161 <= n_fft / 2 + 1 <= 256 can stream (DS2_UNSUPPORTED_SHAPE otherwise:
 * the mirror-fill for fewer bins reads frames ahead of the column it fills).  No masks.
 * State: one opaque device buffer of ds2_stft_stream_state_size(n, n_fft, hop) bytes (0 for
 * arguments no state exists for), 256-byte aligned, owned by the caller: per stream the
 * last min(a, n_fft - 1) samples and samples 0 .. pad as float32, the fp64 sum S_t, the
 * prior and a tag (geometry and samples taken).  ds2_stft_stream_init starts an utterance on
 * all n streams; prior_offset NULL (no prior, w = 0) or n device doubles o0 with weight
 * prior_frames >= 0.
 * ds2_stft_stream_feed:
 *   chunk       [n][chunk_samples] with row stride chunk_stride (elements): dtype 0 float32
 *               in [-1, 1], dtype 1 int16 read as (float)s * scale (2^-15 is exact); may be
 *               NULL when chunk_samples == 0
 *   samples_done  samples fed by earlier calls since init (the caller's count: no call
 *               synchronises); last 0 / 1: the utterance ends with this chunk
 *   window      n_fft doubles; normalize 0 / 1; fixed_offset NULL or [n] floats (normalize 1)
 *   out         [n][161][k], k = the frames this feed makes final; a k other than what
 *               samples_done, chunk_samples and last yield is DS2_INVALID_VALUE
 *   cur_offset  NULL or [n] doubles: S_t / (t + 1) after this feed (o0 before any frame)
 *   out_frames  NULL or [n] int32: frames emitted so far, -1 for a record whose tag does not
 *               match (n_fft, hop, samples_done): such a stream is not advanced and its rows
 *               of out are not written (the tag is on the device, so the host cannot refuse)
 *   ws          ds2_stft_stream_workspace_size(n, k) bytes (normalize 1, k > 0: the frame means)
 * Two launches (one when k == 0), no allocation, no synchronisation.  n == 0, or
 * chunk_samples == 0 without last, is DS2_OK and launches nothing.  DS2_INVALID_VALUE,
 * before anything is launched, also for a NULL or misaligned state and a state_bytes below
 * the size query.  Feeds of one state must be ordered (one stream, or events). */
size_t ds2_stft_stream_state_size(int n, int n_fft, int hop);
size_t ds2_stft_stream_workspace_size(int n, int k);
ds2_status_t ds2_stft_stream_init(void* state, size_t state_bytes, int n, int n_fft, int hop,
                                  const double* prior_offset, double prior_frames,
                                  ds2_stream_t stream);
ds2_status_t ds2_stft_stream_feed(const void* chunk, int dtype, int n, int chunk_samples,
                                  int64_t chunk_stride, float scale, int64_t samples_done,
                                  int last, int n_fft, int hop, const double* window,
                                  int normalize, const float* fixed_offset, float* out, int k,
                                  double* cur_offset, int* out_frames, void* state,
                                  size_t state_bytes, void* ws, size_t ws_bytes,
                                  ds2_stream_t stream);

/* Waveform augmentations before the STFT: replays per-utterance op records drawn on the
 * host by ds2amd/audio_aug.py in the reference's `random` / `np.random` order —
 * Shift (data/audio_aug.py:26-44), AudioDistort (:47-60,177-178), AddNoise (:78-107).
 * in: [n][in_stride] fp32 PCM with in_lens; op_i [n][max_ops][4] = {kind, a, b, 0}
 * (kind 0 end, 1 shift (a = shift, b = limit), 2 distort, 3 noise (a = noise row)),
 * op_f [n][max_ops] = alpha; noise [rows][noise_stride] float64 slices; out:
 * [n][out_stride] zero padded, out_lens = the lengths the host expects (mismatch, a bad
 * record or cap too small sets *err).  cap = the longest intermediate length.  *err is OR-ed
 * with 1 for a length past cap (in_lens itself, or a shift's result) or a shift outside
 * [0, limit], 2 for a record that cannot be replayed (an unknown kind, noise with noise ==
 * NULL), 4 for a final length other than out_lens; such a row leaves out untouched.  Replaces
 * the numpy arithmetic of load_randomly_augmented_audio (data_loader_aug.py:660-699). */
size_t ds2_wave_aug_workspace_size(int n, int64_t cap);
ds2_status_t ds2_wave_aug(const float* in, int64_t in_stride, const int* in_lens, int n,
                          const int* op_i, const double* op_f, int max_ops, const double* noise,
                          int64_t noise_stride, float* out, int64_t out_stride,
                          const int* out_lens, int64_t cap, int* err, void* ws, size_t ws_bytes,
                          ds2_stream_t stream);

/* librosa.effects.time_stretch(y, rate[b]) per utterance (ChangeAudioSpeed, data/audio_aug.py:7-23;
 * the stretch half of PitchShift, :63-75): STFT (n_fft 2048, hop 512, periodic Hann `window`
 * [2048] doubles, reflect pad) -> phase vocoder -> ISTFT, librosa 0.8 semantics (csrc/effects.hip,
 * oracle/librosa_effects.py).  x: [n][x_stride] fp32 with in_lens; per utterance, host-computed:
 * out_frames = ceil((1 + in_len / 512) / rate) (np.arange), used_frames = min(out_frames,
 * ceil((out_len + 2048) / 512)) (istft's `length`), out_lens = round(in_len / rate).  out:
 * [n][out_stride], zero past out_lens.  max_*_frames bound the per-utterance counts. */
size_t ds2_time_stretch_workspace_size(int n, int max_in_frames, int max_out_frames);
ds2_status_t ds2_time_stretch(const float* x, int64_t x_stride, const int* in_lens, int n,
                              const double* rate, const int* out_frames, const int* used_frames,
                              const int* out_lens, const double* window, float* out,
                              int64_t out_stride, int max_in_frames, int max_out_frames, void* ws,
                              size_t ws_bytes, ds2_stream_t stream);
/* resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') per utterance (librosa.resample,
 * data_loader_aug.py:668; the resample half of PitchShift): ratio[b] = sr_new / sr_orig,
 * n_valid[b] = int(in_len * ratio) output samples, zero up to out_stride (librosa's fix_length).
 * win: the filter's right wing (nwin doubles, num_table samples per zero crossing). */
size_t ds2_resample_workspace_size(int n, int64_t max_out);
ds2_status_t ds2_resample(const float* x, int64_t x_stride, const int* in_lens, int n,
                          const double* ratio, const int* n_valid, const double* win, int nwin,
                          int num_table, float* out, int64_t out_stride, void* ws,
                          size_t ws_bytes, ds2_stream_t stream);
/* load_audio (ref data/audio_loader.py:4-27, called at data_loader_aug.py:664,681): the
 * int16 -> float32 conversion, the division by max |x| and the channel selection of a batch of
 * wav files, from their raw samples.  pcm: pcm_elems int16 (2-byte aligned), the interleaved
 * `data` chunks of n files back to back.  desc [n][4] int64 = {first int16 element, frames,
 * channels (1..8), selector (-1 = mean over channels, else a channel index)}, given twice: desc_host
 * in host memory, validated here before any HIP call (the one host read of this header), and
 * desc, the same words in device memory, which the kernels read.  out [n][out_stride] fp32: row
 * b = the mono signal in [0, frames_b), zeros up to out_stride, all written here.  Bit for bit
 * numpy's arithmetic: abs_max = max of np.abs over every channel in int16 (|-32768| wraps to
 * -32768); iff abs_max > 0 a sample is (float)((double)s * (1.0 / (double)abs_max)); the mean is
 * the float32 ndarray.mean(axis=1) (sequential sum, 8-way pairwise at 8 channels, one division).
 * n == 0: DS2_OK, nothing launched; frames == 0: a row of zeros; negative sizes, channels
 * outside 1..8, a selector outside [-1, channels), out_stride < max frames, samples past
 * pcm_elems and NULL pointers: DS2_INVALID_VALUE.  Two launches on `stream`, no sync.       */
size_t ds2_pcm_decode_workspace_size(int n);
ds2_status_t ds2_pcm_decode(const int16_t* pcm, int64_t pcm_elems, const int64_t* desc_host,
                            const int64_t* desc, int n, float* out, int64_t out_stride, void* ws,
                            size_t ws_bytes, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Dense fp32 GEMM on MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2_f32), strided-batched, row-major.
 * C[b] = alpha * op(A[b]) @ op(B[b]) + beta * C[b] (+ bias[n] if bias != NULL)
 * trans_a = 0: A is [m][lda];  1: A is stored [k][lda] (A^T)
 * trans_b = 0: B is [k][ldb];  1: B is stored [n][ldb] (B^T)
 * Replaces cuBLAS behind cuDNN's RNN input projection / BPTT weight gradients
 * (ref model.py:90-91,104 nn.GRU) and nn.Linear (ref model.py:337).
 * lda, ldb, ldc >= the stored row extent and any batch strides (0: one operand shared by the
 * batch; entries of C must not overlap); elements of the allocations outside the logical
 * matrices are neither read into the result nor written.  beta == 0: C is not read.  m, n or
 * batch 0: DS2_OK, nothing done; k == 0 with m, n > 0: DS2_UNSUPPORTED_SHAPE.            */
ds2_status_t ds2_sgemm(int trans_a, int trans_b, int m, int n, int k, float alpha,
                       const float* a, int64_t lda, int64_t stride_a,
                       const float* b, int64_t ldb, int64_t stride_b, float beta,
                       float* c, int64_t ldc, int64_t stride_c, int batch,
                       const float* bias, ds2_stream_t stream);
/* Same with a workspace: when the output grid cannot fill the chip and K is long
 * (weight gradients: M = 3H, N = In, K = T*N), K is split across workgroups and
 * the fp32 partials are reduced in a fixed order (deterministic).  The size query is large
 * enough for any kernel's plan.  A smaller workspace is legal and only slower: one that cannot
 * hold the plan's split slabs is not used at all (as ds2_sgemm), one that holds the slabs but
 * not the (m + n) * 4 + 512 bytes of fp16x3 row-scale words after them runs the bf16x6 kernel. */
size_t ds2_sgemm_workspace_size(int m, int n, int k, int batch);
ds2_status_t ds2_sgemm_ws(int trans_a, int trans_b, int m, int n, int k, float alpha,
                          const float* a, int64_t lda, int64_t stride_a,
                          const float* b, int64_t ldb, int64_t stride_b, float beta,
                          float* c, int64_t ldc, int64_t stride_c, int batch,
                          const float* bias, void* ws, size_t ws_bytes, ds2_stream_t stream);
/* fp16x3 operand scales: row_amax[r] / col_amax[c] = the float bits of max |x| over row r /
 * column c of x [rows][ld] (either output NULL: not computed; non-negative float bits order
 * as unsigned).  16-B aligned x, cols and ld multiples of 4, else DS2_UNSUPPORTED_SHAPE.  One
 * pass over x.  A NaN is skipped (max of the other elements), an inf gives inf.            */
ds2_status_t ds2_amax(const float* x, int rows, int cols, int64_t ld, unsigned* row_amax,
                      unsigned* col_amax, ds2_stream_t stream);
/* ds2_sgemm_ws (batch 1) with the fp16x3 scales of the logical operand rows supplied by the
 * caller: a_amax[m] = max over k of |op(A)[m][k]|, b_amax[n] = max over k of |op(B)[k][n]|
 * (ds2_amax bits; an upper bound is valid and costs only precision below 2^-17 of it: per
 * element |C - C64| <= 2^-20 (|A||B|) + 2^-38 (a_amax (x) sum_k |B| + sum_k |A| (x) b_amax)); NULL
 * = computed here.  Ignored unless the fp16x3 kernel runs.                               */
ds2_status_t ds2_sgemm_amax_ws(int trans_a, int trans_b, int m, int n, int k, float alpha,
                               const float* a, int64_t lda, const float* b, int64_t ldb,
                               float beta, float* c, int64_t ldc, const float* bias,
                               const unsigned* a_amax, const unsigned* b_amax, void* ws,
                               size_t ws_bytes, ds2_stream_t stream);
/* bf16-operand variant (BASELINE cfg4 "bf16 MFMA RNN GEMMs", opt-in): same contract, A and
 * B rounded to bf16 (nearest even) as they are staged, v_mfma_f32_16x16x32_bf16, fp32
 * accumulation and fp32 C.  Needs float4-aligned operands (16-B aligned pointers, ld and
 * the contiguous extent multiples of 4): DS2_UNSUPPORTED_SHAPE otherwise. */
size_t ds2_sgemm_bf16_workspace_size(int m, int n, int k, int batch);
ds2_status_t ds2_sgemm_bf16_ws(int trans_a, int trans_b, int m, int n, int k, float alpha,
                               const float* a, int64_t lda, int64_t stride_a,
                               const float* b, int64_t ldb, int64_t stride_b, float beta,
                               float* c, int64_t ldc, int64_t stride_c, int batch,
                               const float* bias, void* ws, size_t ws_bytes,
                               ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Conv2d, NCHW fp32, on MFMA. ref model.py:209,212 (nn.Conv2d via cuDNN), masked
 * by MaskConv model.py:63-79 when out_lens != NULL: output columns w >= out_lens[n]
 * are written as 0.  Width-stride-1 convolutions (conv2) run as direct
 * convolutions from LDS input patches and need the workspace (re-laid-out
 * filter taps); others (conv1) run as an implicit GEMM and ignore it.
 * Alignment: x, w, bias, dy, y, dx, dw and dbias need 4 bytes only (every kernel reads and
 * writes them one float at a time; the fp16x3 sample maximum takes 16-byte loads only where a
 * sample starts 16-byte aligned); the workspace must be 256-byte aligned (its sections are
 * read with 16-byte loads at offsets that are multiples of 256).  out_lens[n] <= 0 gives an
 * all-zero sample, out_lens[n] >= the output width masks nothing.  n == 0: DS2_OK, nothing
 * launched; a size or stride < 1, a negative padding, or a kernel larger than the padded input
 * (no output row or column): DS2_INVALID_VALUE; a workspace smaller than the plan of the call
 * needs (never more than the size query): DS2_WORKSPACE_TOO_SMALL, nothing launched.       */
size_t ds2_conv2d_workspace_size(int n, int c_in, int h_in, int w_in, int c_out, int kh, int kw,
                                 int sh, int sw, int ph, int pw);
ds2_status_t ds2_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                            int n, int c_in, int h_in, int w_in, int c_out, int kh, int kw,
                            int sh, int sw, int ph, int pw, const int* out_lens, void* ws,
                            size_t ws_bytes, ds2_stream_t stream);
ds2_status_t ds2_conv2d_dgrad(const float* dy, const float* w, float* dx,
                              int n, int c_in, int h_in, int w_in, int c_out, int kh, int kw,
                              int sh, int sw, int ph, int pw, void* ws, size_t ws_bytes,
                              ds2_stream_t stream);
size_t ds2_conv2d_wgrad_workspace_size(int n, int c_in, int h_in, int w_in, int c_out, int kh,
                                       int kw, int sh, int sw, int ph, int pw);
/* dw = sum over (n, ho, wo) of dy * im2col(x); dbias = sum of dy (if dbias != NULL). */
ds2_status_t ds2_conv2d_wgrad(const float* dy, const float* x, float* dw, float* dbias,
                              int n, int c_in, int h_in, int w_in, int c_out, int kh, int kw,
                              int sh, int sw, int ph, int pw, void* ws, size_t ws_bytes,
                              ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Conv1d of the Wav2Letter acoustic model (rnn_type 'cnn'): nn.Conv1d semantics, dilation 1,
 * groups 1, on time-major activations.  ref model.py:518-520 (nn.Conv1d in Wav2Letter's
 * _block via cuDNN), model.py:233 (the fc Conv1d), called at model.py:351-352.
 *   x [t][n][c_in] -> y [t_out][n][c_out],  t_out = (t + 2 p - k) / s + 1;  w [c_out][c_in][k]
 * (torch's layout), bias [c_out] or NULL.  Zero padding is predicated in the loaders.
 * Default: an implicit GEMM on the fp16x3 matrix-core products (fp32-class accuracy; the
 * weights are re-laid into the workspace and the operand scales computed there per call);
 * k = 1, s = 1, p = 0 runs on ds2_sgemm_ws; shapes the implicit GEMM declines (channel
 * counts below 16, dgrad with s > 1) and DS2_CONV1D=0 run general fp32 FMA kernels.
 * t == 0 or n == 0: DS2_OK, nothing launched; negative sizes, k or s < 1 and t_out <= 0
 * (t + 2 p - k < 0): DS2_INVALID_VALUE, and the size queries return 0.  One workspace size
 * serves forward and dgrad.
 * Alignment: x, w, bias, dy, y, dx, dw and dbias need 4 bytes only.  The implicit GEMM reads
 * the activations it gathers (x; dy in dgrad) with 16-byte loads only where their address is
 * 16-byte aligned and their channel count a multiple of 4, one float at a time otherwise;
 * every other kernel of the family reads and writes the caller's arrays one float at a time.
 * The workspace must be 256-byte aligned (its sections are read with 16-byte loads); what it
 * holds on entry does not matter.  Caller-supplied maxima (the _amax entries) need 4 bytes.
 * Workspace: every call checks for what the kernel it chose uses, never more than the size
 * query, and returns DS2_WORKSPACE_TOO_SMALL before anything is launched.  NULL is taken by
 * forward and dgrad where they run the general kernels or ds2_sgemm_ws (k = 1, s = 1, p = 0: a
 * smaller workspace is only slower there), and by every empty call; ds2_conv1d_wgrad always
 * needs its size query's bytes unless the batch is empty.                       */
size_t ds2_conv1d_workspace_size(int t, int n, int c_in, int c_out, int k, int s, int p);
ds2_status_t ds2_conv1d_fwd(const float* x, const float* w, const float* bias, float* y, int t,
                            int n, int c_in, int c_out, int k, int s, int p, void* ws,
                            size_t ws_bytes, ds2_stream_t stream);
/* The same with the fp16x3 row scales of x supplied by its producer: x_row_amax [t n] = the
 * float bits of max |x| per row (ds2_amax's format, e.g. from ds2_bn_relu_apply_amax; an upper
 * bound is valid); NULL = computed here.  Ignored unless the implicit GEMM runs.          */
ds2_status_t ds2_conv1d_fwd_amax(const float* x, const float* w, const float* bias, float* y,
                                 int t, int n, int c_in, int c_out, int k, int s, int p,
                                 const unsigned* x_row_amax, void* ws, size_t ws_bytes,
                                 ds2_stream_t stream);
/* dx [t][n][c_in] from dy [t_out][n][c_out] (autograd of model.py:351; overwritten). */
ds2_status_t ds2_conv1d_dgrad(const float* dy, const float* w, float* dx, int t, int n, int c_in,
                              int c_out, int k, int s, int p, void* ws, size_t ws_bytes,
                              ds2_stream_t stream);
/* dw [c_out][c_in][k] = sum over (t_out, n) of dy * window(x); dbias [c_out] = column sums of
 * dy (if dbias != NULL).  Both overwritten; deterministic: K = t_out n is split into slabs
 * whose fp32 partials are summed in a fixed order, as ds2_sgemm_ws does.            */
size_t ds2_conv1d_wgrad_workspace_size(int t, int n, int c_in, int c_out, int k, int s, int p);
ds2_status_t ds2_conv1d_wgrad(const float* dy, const float* x, float* dw, float* dbias, int t,
                              int n, int c_in, int c_out, int k, int s, int p, void* ws,
                              size_t ws_bytes, ds2_stream_t stream);
/* x [n][c][t] -> y [t][n][c]: the spectrogram batch [N][1][161][T] (ref model.py:350
 * x.squeeze(1)) into the time-major layout the Conv1d kernels read, one pass.        */
ds2_status_t ds2_nct_to_tnc(const float* x, int n, int c, int t, float* y, ds2_stream_t stream);
/* ds2_conv1d_wgrad with the column maxima of x supplied (x_col_amax [c_in], as above). */
ds2_status_t ds2_conv1d_wgrad_amax(const float* dy, const float* x, float* dw, float* dbias, int t,
                                   int n, int c_in, int c_out, int k, int s, int p,
                                   const unsigned* x_col_amax, void* ws, size_t ws_bytes,
                                   ds2_stream_t stream);
/* GLU over channels, x [rows][2 c] -> y [rows][c] = a * sigmoid(b), a the first c channels
 * (ref model.py:529 GLUModule(dim=1) = F.glu on [N][2C][T]), and its backward dx [rows][2 c]. */
ds2_status_t ds2_glu_fwd(const float* x, int rows, int c, float* y, ds2_stream_t stream);
ds2_status_t ds2_glu_bwd(const float* dy, const float* x, int rows, int c, float* dx,
                         ds2_stream_t stream);
/* BatchNorm1d apply + ReLU in one pass over [rows][c] (ref model.py:524,527: BatchNorm1d then
 * ReLU over (N, T) per channel; statistics from ds2_bn_train_stats / ds2_bn_eval_stats with
 * inner = 1): y = max(gamma (x - mean) invstd + beta, 0).  Backward: dz = dy where y > 0,
 * then the training-mode BatchNorm backward of ds2_bn_backward (dx, dgamma, dbeta
 * overwritten; dx may not alias dy).                                               */
ds2_status_t ds2_bn_relu_apply(const float* x, int rows, int c, const float* mean,
                               const float* invstd, const float* gamma, const float* beta,
                               float* y, ds2_stream_t stream);
/* ds2_bn_relu_apply that also writes the fp16x3 scales of y in the same pass, as
 * ds2_bn_apply_amax does (same shape conditions: c % 4 == 0, c <= 2048, 16-B aligned
 * operands, else DS2_UNSUPPORTED_SHAPE): row_amax [rows] for the next Conv1d's forward,
 * col_amax [c] for its weight gradient.                                              */
ds2_status_t ds2_bn_relu_apply_amax(const float* x, int rows, int c, const float* mean,
                                    const float* invstd, const float* gamma, const float* beta,
                                    float* y, unsigned* row_amax, unsigned* col_amax,
                                    ds2_stream_t stream);
size_t ds2_bn_relu_bwd_workspace_size(int rows, int c);
ds2_status_t ds2_bn_relu_bwd(const float* dy, const float* y, const float* x, int rows, int c,
                             const float* mean, const float* invstd, const float* gamma,
                             const float* beta, float* dx, float* dgamma, float* dbeta, void* ws,
                             size_t ws_bytes, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Dropout of the Wav2Letter blocks (ref model.py:535-536: nn.Dropout appended to every block
 * when --dropout > 0), training mode.  No mask is stored: element i of the row-major
 * [rows][c] matrix (i = r c + col, 64-bit) is decided by a counter-based stream,
 *   Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85),
 *   key     = (seed & 0xffffffff, seed >> 32),
 *   counter = (g & 0xffffffff, g >> 32, offset & 0xffffffff, offset >> 32),  g = i / 4,
 *   word    = output word i % 4 of that call,
 *   thr     = floor(p * 2^32) in double;  element i is dropped iff word < thr,
 * and y[i] = dropped ? 0 : x[i] * scale with scale = 1.0f / (1.0f - p) in float (one float
 * multiply, torch's formula).  p == 0 is the identity, p == 1 writes zeros.  The same
 * (seed, offset) gives the same mask on every call, so a backward regenerates it; a caller
 * advances offset between masks (ds2amd: by 4, torch's generator granularity).  These masks
 * are not the ones torch's native dropout draws under the same seed.
 * Every entry: p outside [0, 1] or NaN and negative sizes are DS2_INVALID_VALUE before any
 * HIP call; rows == 0 or c == 0 is DS2_OK with nothing launched.                        */
/* y = dropout(x), any c and alignment (y may alias x).  The backward is the same call on dy.
 * ref model.py:535-536.                                                                  */
ds2_status_t ds2_dropout_apply(const float* x, int rows, int c, float p, uint64_t seed,
                               uint64_t offset, float* y, ds2_stream_t stream);
/* BatchNorm1d apply [+ ReLU if relu != 0] + dropout in one pass, with the fp16x3 scales of
 * the y it stored (row_amax [rows], col_amax [c]) as ds2_bn_relu_apply_amax /
 * ds2_bn_apply_amax write them: y = dropout(act(gamma (x - mean) invstd + beta)), the affine
 * and ReLU bit for bit those entries'.  Same shape conditions (c % 4 == 0, c <= 2048, 16-B
 * aligned operands, else DS2_UNSUPPORTED_SHAPE).  ref model.py:535-536 after 524-531.    */
ds2_status_t ds2_bn_dropout_apply_amax(const float* x, int rows, int c, const float* mean,
                                       const float* invstd, const float* gamma,
                                       const float* beta, int relu, float p, uint64_t seed,
                                       uint64_t offset, float* y, unsigned* row_amax,
                                       unsigned* col_amax, ds2_stream_t stream);
/* Backward of the relu != 0 form from its stored output y: y > 0 already means "passed the
 * ReLU and kept", so dz = dy * scale where y > 0 (else 0), then ds2_bn_backward as
 * ds2_bn_relu_bwd does (workspace ds2_bn_relu_bwd_workspace_size; dx may not alias dy).
 * The relu == 0 form's backward is ds2_dropout_apply on dy, then ds2_bn_backward.
 * ref model.py:535-536.                                                                  */
ds2_status_t ds2_bn_relu_dropout_bwd(const float* dy, const float* y, const float* x, int rows,
                                     int c, const float* mean, const float* invstd,
                                     const float* gamma, const float* beta, float p, float* dx,
                                     float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                     ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* BatchNorm (training statistics), x viewed as [outer][c][inner].
 * ref model.py:210,213 (BatchNorm2d), model.py:89,336 (SequenceWise BatchNorm1d).
 * Batch statistics include padded (zeroed) positions, as in the reference.
 * Computes save_mean / save_invstd and updates the running stats in place
 * (running_var uses the unbiased variance, momentum as in torch).            */
size_t ds2_bn_workspace_size(int outer, int c, int inner);
ds2_status_t ds2_bn_train_stats(const float* x, int outer, int c, int inner, float eps,
                                float momentum, float* save_mean, float* save_invstd,
                                float* running_mean, float* running_var, void* ws,
                                size_t ws_bytes, ds2_stream_t stream);
ds2_status_t ds2_bn_eval_stats(const float* running_mean, const float* running_var, int c,
                               float eps, float* save_mean, float* save_invstd,
                               ds2_stream_t stream);
/* y = gamma * (x - mean) * invstd + beta over [outer][c][inner]. */
ds2_status_t ds2_bn_apply(const float* x, int outer, int c, int inner, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, float* y,
                          ds2_stream_t stream);
/* ds2_bn_apply over [rows][c] (inner 1) that also writes the fp16x3 GEMM scales of y: the
 * float bits of max |y| per row (row_amax[rows]) and per column (col_amax[c]), the next
 * input projection's A-row and dW_ih's B-column maxima (ds2_sgemm_amax_ws).  Needs c % 4 == 0,
 * c <= 2048 and 16-B aligned x / y / mean / invstd / gamma / beta (DS2_UNSUPPORTED_SHAPE
 * otherwise).  Replaces the same SequenceWise BatchNorm1d as ds2_bn_apply (model.py:89). */
ds2_status_t ds2_bn_apply_amax(const float* x, int rows, int c, const float* mean,
                               const float* invstd, const float* gamma, const float* beta,
                               float* y, unsigned* row_amax, unsigned* col_amax,
                               ds2_stream_t stream);
/* Conv-block epilogue (MaskConv, model.py:69-78): x is [n][c][d][t];
 * y = mask(hardtanh(mask(bn(x)), lo, hi)) where mask zeroes t >= lens[n].
 * out_layout 0: y is [n][c][d][t];  1: y is [t][n][c*d] (the TxNxH collapse of
 * model.py:360-362, fused).                                                   */
ds2_status_t ds2_bn_apply_mask_htanh(const float* x, int n, int c, int d, int t,
                                     const float* mean, const float* invstd, const float* gamma,
                                     const float* beta, const int* lens, float lo, float hi,
                                     float* y, int out_layout, ds2_stream_t stream);
/* Backward of bn_apply (masked == 0, x viewed [outer][c][d*t]) or of
 * bn_apply_mask_htanh (masked != 0, x is [outer=n][c][d][t], lens/lo/hi as in
 * the forward).  dy has the layout of the forward output (dy_layout as
 * out_layout above; layout 1 only with masked != 0).  Writes dx
 * ([outer][c][d][t]), dgamma, dbeta (overwritten) and, if dbias_in != NULL, the
 * gradient of the per-channel bias added before the masked BN (the conv bias;
 * exact closed form, see bn.hip).  dx may not alias dy.  eps: the forward's, or
 * <= 0 if not known.  With it, channels of at most 8 values take invstd from x in
 * fp64 and not from the float `invstd`, whose rounding is percents of dx when a
 * channel holds 2 values (dx ~ eps invstd^2 there); larger channels and the mask
 * decisions always use the stored floats.                                     */
ds2_status_t ds2_bn_backward(const float* dy, int dy_layout, const float* x, int outer, int c,
                             int d, int t, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, int masked,
                             const int* lens, float lo, float hi, float eps, float* dx,
                             float* dgamma, float* dbeta, float* dbias_in, void* ws,
                             size_t ws_bytes, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Bidirectional GRU recurrence (torch gate order r, z, n), packed-sequence
 * semantics: direction 0 runs t = 0..len-1, direction 1 runs t = len-1..0,
 * both from h = 0; outputs at t >= len are 0.  ref model.py:97-109 (BatchRNN
 * pack -> nn.GRU -> pad), model.py:16 (supported_rnns['gru']).
 *   xproj : [T][N][D][3H]  x @ W_ih^T + b_ih for each direction
 *   h_all : [T][N][D][H]   per-direction hidden states (output)
 *   gates : the backward cache, or NULL: ds2_gru_cache_floats(T, N, H, D) floats =
 *           [T][N][D][4H] (r, z, n, W_hn h + b_hn)
 * num_dirs = 1 or 2; w_hh_r / b_hh_r ignored when num_dirs == 1.
 * err_out: NULL, or a caller-owned device status word; the persistent
 * (one-launch-per-layer) kernels OR their hand-off status into it after the
 * launch (DS2_RNN_ERR_HANDOFF_TIMEOUT: a workgroup waited past the spin bound,
 * its outputs from that step on are NaN).  The word is never cleared by the
 * library, so one word can collect a whole training step; the caller reads
 * it whenever it synchronises anyway (same convention for ds2_gru_bwd and
 * ds2_lstm_fwd / ds2_lstm_bwd).                                               */
#define DS2_RNN_ERR_HANDOFF_TIMEOUT 1u
size_t ds2_gru_cache_floats(int t_max, int n, int h, int num_dirs);
size_t ds2_gru_fwd_workspace_size(int n, int h, int num_dirs);
ds2_status_t ds2_gru_fwd(int t_max, int n, int h, int num_dirs, const float* xproj,
                         const float* w_hh_f, const float* w_hh_r, const float* b_hh_f,
                         const float* b_hh_r, const int* lens, float* h_all, float* gates,
                         unsigned* err_out, void* ws, size_t ws_bytes, ds2_stream_t stream);
/* ds2_gru_fwd from an initial hidden state (chunked / streaming inference of a unidirectional
 * layer).  The two state arguments stand between `gates` and `err_out`:
 *   h0     : [N][H]    the state before step 0
 *   hproj0 : [N][3H]   h0 @ W_hh^T WITHOUT b_hh -- the caller's GEMM, as xproj is
 * Only step 0 differs from ds2_gru_fwd: it adds hproj0 where the in-kernel W_hh product of the
 * later steps stands and takes h_prev = h0.  The kernel is chosen by the shape exactly as
 * without a state, and the workspace is ds2_gru_fwd_workspace_size's.  Both NULL: exactly
 * ds2_gru_fwd.  One of the two NULL, or a state with num_dirs != 1: DS2_INVALID_VALUE, nothing
 * launched.  A sample's final state is row len - 1 of h_all (rows t >= len are 0 as before);
 * len = 0 leaves no row to read.                                                          */
ds2_status_t ds2_gru_fwd_state(int t_max, int n, int h, int num_dirs, const float* xproj,
                               const float* w_hh_f, const float* w_hh_r, const float* b_hh_f,
                               const float* b_hh_r, const int* lens, float* h_all, float* gates,
                               const float* h0, const float* hproj0, unsigned* err_out, void* ws,
                               size_t ws_bytes, ds2_stream_t stream);
size_t ds2_gru_bwd_workspace_size(int n, int h, int num_dirs);
/* dy: [T][N][dy_dirs][H]; dy_dirs = 1: gradient of the direction-summed output
 * (model.py:107), dy_dirs = num_dirs: per-direction output gradient.
 * dgates_x: [T][N][D][3H] grad wrt xproj;  dgates_h: [T][N][D][3H] grad wrt
 * W_hh h + b_hh.  Weight gradients are then plain GEMMs (see ds2amd/ops.py). */
ds2_status_t ds2_gru_bwd(int t_max, int n, int h, int num_dirs, const float* dy, int dy_dirs,
                         const float* w_hh_f, const float* w_hh_r, const float* h_all,
                         const float* gates, const int* lens, float* dgates_x, float* dgates_h,
                         unsigned* err_out, void* ws, size_t ws_bytes, ds2_stream_t stream);
/* Workgroups the persistent backward recurrence holds at once for this shape (one per
 * CU, all resident together: they spin on each other's hand-offs; an upper bound when the
 * launch may fall back to another persistent kernel), 0 when the shape runs the per-step
 * kernels.  What a concurrent collective must leave free (DESIGN.md §6;
 * optim.GradAllReducer.guard_cooperative).                                     */
int ds2_gru_bwd_grid(int n, int h, int num_dirs);
int ds2_lstm_bwd_grid(int n, int h, int num_dirs);
/* ds2_gru_bwd plus the bias gradients of the layer (replaces the column sums of the
 * reference's autograd over bias_ih_l* / bias_hh_l*, nn.GRU via model.py:97-109):
 * db_ih_{f,r} [3H] = sum over rows of dgates_x, db_hh_{f,r} [3H] = sum over rows of
 * dgates_h.  The direct-operand backward sums them while it runs (fp64, fixed order);
 * other recurrence paths sum dgates_x / dgates_h afterwards.  db_ih_f == NULL: same as
 * ds2_gru_bwd; with num_dirs == 1 the _r pointers may be NULL.                 */
ds2_status_t ds2_gru_bwd_bias(int t_max, int n, int h, int num_dirs, const float* dy, int dy_dirs,
                              const float* w_hh_f, const float* w_hh_r, const float* h_all,
                              const float* gates, const int* lens, float* dgates_x,
                              float* dgates_h, float* db_ih_f, float* db_hh_f, float* db_ih_r,
                              float* db_hh_r, unsigned* err_out, void* ws, size_t ws_bytes,
                              ds2_stream_t stream);
/* ds2_gru_bwd_bias plus the column maxima of the gate gradients for the fp16x3 GEMMs that
 * follow (ds2_sgemm_amax_ws: dW_ih, dW_hh): col_amax[0, D 3H) = max over rows of |dgates_x|,
 * [D 3H, 2 D 3H) = the same of dgates_h, as float bits (ds2_amax's format).  The fp16x3
 * recurrence keeps them as it goes; any other kernel is followed by a column pass, so D 3H
 * must be a multiple of 4 as for ds2_amax (DS2_UNSUPPORTED_SHAPE otherwise, nothing launched:
 * call ds2_gru_bwd_bias). */
ds2_status_t ds2_gru_bwd_bias_amax(int t_max, int n, int h, int num_dirs, const float* dy,
                                   int dy_dirs, const float* w_hh_f, const float* w_hh_r,
                                   const float* h_all, const float* gates, const int* lens,
                                   float* dgates_x, float* dgates_h, float* db_ih_f,
                                   float* db_hh_f, float* db_ih_r, float* db_hh_r,
                                   unsigned* col_amax, unsigned* err_out, void* ws,
                                   size_t ws_bytes, ds2_stream_t stream);
/* The row maxima of dgates_x ([T N] float bits, ds2_amax's row format: the dX GEMM's row
 * scales) without a pass over dgates_x.  When ds2_gru_bwd_bias_amax is given a workspace of
 * ds2_gru_row_amax_workspace_size(T, N, H, D) bytes (>= ds2_gru_bwd_workspace_size), the
 * XCD-local fp16x3 recurrence leaves per-workgroup partial maxima behind in it, and
 * ds2_gru_row_amax -- called next on the same stream with the same shape and workspace --
 * reduces them; rows with t >= len are 0.  DS2_UNSUPPORTED_SHAPE when that workspace holds no
 * partials of such a call (another recurrence kernel ran, or the workspace was the smaller
 * one): the caller then takes ds2_amax over dgates_x, which gives the same bits.          */
size_t ds2_gru_row_amax_workspace_size(int t_max, int n, int h, int num_dirs);
ds2_status_t ds2_gru_row_amax(int t_max, int n, int h, int num_dirs, const void* ws,
                                  size_t ws_bytes, unsigned* row_amax, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* (Bi)directional LSTM recurrence (torch gate order i, f, g, o), same packed-
 * sequence semantics as the GRU.  ref model.py:14 (supported_rnns['lstm'] =
 * nn.LSTM) inside BatchRNN model.py:97-109.
 *   xproj : [T][N][D][4H]  x @ W_ih^T + b_ih for each direction
 *   h_all : [T][N][D][H]   hidden states (output)
 *   c_all : [T][N][D][H]   cell states (backward cache, or NULL)
 *   gates : [T][N][D][4H]  activated (i, f, g, o) cache for backward, or NULL  */
size_t ds2_lstm_fwd_workspace_size(int n, int h, int num_dirs);
ds2_status_t ds2_lstm_fwd(int t_max, int n, int h, int num_dirs, const float* xproj,
                          const float* w_hh_f, const float* w_hh_r, const float* b_hh_f,
                          const float* b_hh_r, const int* lens, float* h_all, float* c_all,
                          float* gates, unsigned* err_out, void* ws, size_t ws_bytes,
                          ds2_stream_t stream);
/* ds2_lstm_fwd from an initial state, as ds2_gru_fwd_state: between `gates` and `err_out`
 * stand h0 [N][H], c0 [N][H] and hproj0 [N][4H] = h0 @ W_hh^T (no bias).  All three NULL:
 * exactly ds2_lstm_fwd; a partial set, or a state with num_dirs != 1: DS2_INVALID_VALUE,
 * nothing launched.  The final state is row len - 1 of h_all and of c_all (a caller that
 * carries on passes a c_all buffer).                                                      */
ds2_status_t ds2_lstm_fwd_state(int t_max, int n, int h, int num_dirs, const float* xproj,
                                const float* w_hh_f, const float* w_hh_r, const float* b_hh_f,
                                const float* b_hh_r, const int* lens, float* h_all, float* c_all,
                                float* gates, const float* h0, const float* c0,
                                const float* hproj0, unsigned* err_out, void* ws,
                                size_t ws_bytes, ds2_stream_t stream);
size_t ds2_lstm_bwd_workspace_size(int n, int h, int num_dirs);
/* dy as for ds2_gru_bwd.  dgates: [T][N][D][4H] gradient wrt the gate
 * pre-activations (= wrt xproj and wrt W_hh h + b_hh).                       */
ds2_status_t ds2_lstm_bwd(int t_max, int n, int h, int num_dirs, const float* dy, int dy_dirs,
                          const float* w_hh_f, const float* w_hh_r, const float* c_all,
                          const float* gates, const int* lens, float* dgates, unsigned* err_out,
                          void* ws, size_t ws_bytes, ds2_stream_t stream);
/* ds2_lstm_bwd for BASELINE cfg4's opt-in bf16 mode (rnn_gemm_precision='bf16'): the W_hh^T
 * product of the backward recurrence on ONE fp16 term per operand (per-row scaled gate
 * gradients, per-column scaled W_hh^T: 11 significant bits each), so a workgroup takes 32
 * samples and cfg4's batch 64 runs as one launch.  Same arguments and workspace as
 * ds2_lstm_bwd, which it falls back to where it declines the shape.
 * ds2_lstm_bwd_half_grid: workgroups that launch holds at once.                          */
int ds2_lstm_bwd_half_grid(int n, int h, int num_dirs);
ds2_status_t ds2_lstm_bwd_half(int t_max, int n, int h, int num_dirs, const float* dy, int dy_dirs,
                               const float* w_hh_f, const float* w_hh_r, const float* c_all,
                               const float* gates, const int* lens, float* dgates,
                               unsigned* err_out, void* ws, size_t ws_bytes, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Lookahead convolution, ref model.py:140-177 (Lookahead.forward), optionally
 * fused with the Hardtanh that follows it (model.py:329-333):
 *   y[t][n][h] = sum_{j=0..context} w[h][j] * x[t+j][n][h]  (0 past T)
 *   clamp != 0: y = min(max(y, lo), hi).   x, y: [T][N][H]; w: [H][context+1];
 *   context + 1 <= 32.                                                       */
ds2_status_t ds2_lookahead_fwd(const float* x, int t, int n, int h, const float* w, int context,
                               int clamp, float lo, float hi, float* y, ds2_stream_t stream);
/* Backward: y = the clamped forward output (or NULL when not clamped: dz = dy,
 * else dz = dy where lo < y < hi).  dx (or NULL) overwritten; dw (or NULL)
 * overwritten, deterministic (exact zeros when t == 0 or n == 0).  The workspace is
 * needed for dw only.  A NULL dy or w, or a NULL x when dw is asked for, is
 * DS2_INVALID_VALUE.  ds2_dirsum, ds2_colsum, ds2_softmax_tnc[_bwd], ds2_greedy_decode,
 * ds2_nan_guard, ds2_zero_masked and ds2_scale_by_device_scalar likewise refuse, before
 * they launch, a NULL data pointer they would dereference, and return DS2_OK whatever
 * the pointers when there is no work.                                           */
size_t ds2_lookahead_bwd_workspace_size(int t, int n, int h, int context);
ds2_status_t ds2_lookahead_bwd(const float* dy, const float* y, float lo, float hi,
                               const float* x, int t, int n, int h, const float* w, int context,
                               float* dx, float* dw, void* ws, size_t ws_bytes,
                               ds2_stream_t stream);

/* y[t][n][j] = sum_d h_all[t][n][d][j]   (model.py:107 view(T,N,2,H).sum(2)) */
ds2_status_t ds2_dirsum(const float* h_all, int rows, int num_dirs, int h, float* y,
                        ds2_stream_t stream);
/* out[j] (+)= sum_i x[i*ld + j]  for i < rows, j < cols (bias gradients). */
size_t ds2_colsum_workspace_size(int rows, int cols);
ds2_status_t ds2_colsum(const float* x, int rows, int cols, int64_t ld, float* out,
                        int accumulate, void* ws, size_t ws_bytes, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Softmax over C of logits stored [T][N][C] -> probs [N][T][C] (model.py:375-377). */
ds2_status_t ds2_softmax_tnc(const float* logits, int t_max, int n, int c, float* probs,
                             ds2_stream_t stream);
/* Backward of ds2_softmax_tnc: dlogits[T][N][C] (+)= y * (dy - sum(y*dy)). */
ds2_status_t ds2_softmax_tnc_bwd(const float* probs, const float* dprobs, int t_max, int n,
                                 int c, float* dlogits, int accumulate, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* CTC loss, warp-ctc semantics (ref train.py:12,600-602 warpctc_pytorch.CTCLoss):
 * softmax is applied internally to acts [T][N][C]; costs[b] = -log p(l_b | x_b);
 * grads [T][N][C] = d cost_b / d acts (softmax - posterior), zero for t >= len.
 * labels: concatenated int32 targets; label_lens[b] their lengths.
 * Infeasible samples (L + repeats > act_len) get cost +inf and zero gradient,
 * or cost 0 when zero_infinity != 0.                                          */
size_t ds2_ctc_workspace_size(int t_max, int n, int max_label_len);
ds2_status_t ds2_ctc_loss(const float* acts, int t_max, int n, int c, const int* labels,
                          const int* label_lens, const int* act_lens, int max_label_len,
                          int blank, int zero_infinity, float* costs, float* grads, void* ws,
                          size_t ws_bytes, ds2_stream_t stream);

/* CTC forced alignment (Viterbi): the best frame-level alignment of a known transcript.
 * Inputs, limits (c <= 64, max_label_len <= 1024) and status codes are those of
 * ds2_ctc_loss; softmax is applied internally.  Per utterance b, with
 * T = clamp(act_lens[b], 0, t_max), L = label_lens[b] and S = 2 L + 1 extended states
 * (even s: blank, odd s: labels[s >> 1]), the alignment is the state sequence
 * s_0 .. s_{T-1} that maximises sum_t log p[t][l'(s_t)] with s_0 in {0, 1}, s_{T-1} in
 * {S - 2, S - 1} and steps of +0, +1 or +2, the +2 step only onto a non-blank state whose
 * label differs from the one two states back.
 * states [n][t_max]: s_t for t < T, -1 for t >= T.
 * spans  [sum of label_lens][2]: for label i of utterance b (row label offset + i) the
 *   first frame in state 2 i + 1 and one past the last.
 * scores [n]: the path's log-probability (0 for T = 0, L = 0).
 * An infeasible utterance (L + repeats > T) gets score -inf and -1 in all of its states
 * and spans.
 * Ties: a predecessor replaces the best so far only if strictly greater, and the
 * predecessors are tried in the order stay, s - 1, s - 2; the final state is S - 1 unless
 * v(S - 2) > v(S - 1).  Deterministic: two calls give bit-identical outputs.
 * Workspace: the log-softmax rows plus one back-pointer byte per (b, t, s).      */
size_t ds2_ctc_align_workspace_size(int t_max, int n, int max_label_len);
ds2_status_t ds2_ctc_align(const float* acts, int t_max, int n, int c, const int* labels,
                           const int* label_lens, const int* act_lens, int max_label_len,
                           int blank, int* states, int* spans, float* scores, void* ws,
                           size_t ws_bytes, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* GreedyDecoder.decode (ref decoder.py:182-197, process_string :165-180):
 * argmax over C (first maximum) of probs[n][t][c] (strides in elements), then
 * drop blanks and frames equal to the previous frame.  Emits compacted label
 * ids and their frame offsets per utterance plus counts[n].                   */
ds2_status_t ds2_greedy_decode(const float* probs, int n, int t_max, int c, int64_t stride_n,
                               int64_t stride_t, const int* sizes, int blank, int* out_ids,
                               int* out_offsets, int* out_counts, int* argmax_out,
                               ds2_stream_t stream);

/* CTC prefix beam search without a language model: BeamCTCDecoder.decode
 * (decoder.py:90-143, ctcdecode.CTCBeamDecoder with lm_path=None; opts.py beam
 * defaults).  probs as for ds2_greedy_decode; per utterance the top_paths best
 * prefixes (best first): out_ids / out_offsets [n][top_paths][t_max] (char ids and
 * the frame of each char), out_lens [n][top_paths], out_scores [n][top_paths]
 * (log prob).  cutoff_top_n / cutoff_prob prune the vocabulary per frame as
 * ctcdecode does.  beam_width <= 128 and c <= 64 (three kernel instances:
 * beam_width <= 32 with c <= 64; beam_width <= 128 with c <= 32, the reference
 * default beam_width = 100 over 29 labels; and 33..128 over 33..64, its Cyrillic
 * label set of 36); anything beyond is DS2_UNSUPPORTED_SHAPE.                 */
/* Batched CER / WER edit distances (data/utils.py:47-57 get_cer_wer, decoder.py
 * Decoder.cer / .wer) over id sequences: a = decoded ids [n][a_stride] with a_lens,
 * b = reference ids flat with b_offsets / b_lens.  out[4*i .. 4*i+3] = {word
 * distance, char distance (spaces removed), max(#reference words, 1),
 * max(#reference non-space chars, 1)}.  The limits count what the distances run over:
 * a sequence with more than 2048 non-space ids or more than 1024 words (either side) sets
 * *err != 0 and both of its pair's distances to -1, with the two reference counts still
 * right; spaces do not count, so a longer raw sequence is accepted.  The other pairs of
 * the launch are scored as usual.  err must be zeroed by the caller.          */
ds2_status_t ds2_edit_distance(const int* a_ids, int64_t a_stride, const int* a_lens,
                               const int* b_ids, const int* b_offsets, const int* b_lens, int n,
                               int space_id, int* out, int* err, ds2_stream_t stream);

size_t ds2_ctc_beam_workspace_size(int n, int t_max, int beam_width);
ds2_status_t ds2_ctc_beam_decode(const float* probs, int n, int t_max, int c, int64_t stride_n,
                                 int64_t stride_t, const int* sizes, int blank, int beam_width,
                                 int cutoff_top_n, double cutoff_prob, int top_paths,
                                 int* out_ids, int* out_offsets, int* out_lens,
                                 float* out_scores, void* ws, size_t ws_bytes,
                                 ds2_stream_t stream);

/* The same search with a word n-gram language model: BeamCTCDecoder(labels, lm_path,
 * alpha, beta, ...) (decoder.py:90-99 -> ctcdecode's KenLM Scorer; opts.py:6-10
 * --lm-path / --alpha / --beta).  A space extension adds float(alpha * ln p(word |
 * preceding order-1 words, "<s>" padded)) and beta; extensions follow the vocabulary
 * trie; once the beam is full a (prefix, char) below worst + log p_blank - max(0, beta)
 * is skipped; the last partial word is scored after the final frame
 * (oracle/ctc_beam_lm.py restates it).  Tables (device memory, ds2amd/lm.py builds them
 * from an ARPA file): dict_next int32 [dict_states][c] trie arcs (-1 none; state 0 =
 * start, dict_states-1 = after a word's space), dict_mask uint64 [dict_states] the arcs
 * as char bits, dict_word int32 [dict_states] the word id a state spells (-1 none);
 * lm_table int32 [lm_slots][8] {w0..w5 (-1 padded), log10 prob bits, log10 backoff
 * bits}, w0 = -1 marks an empty slot, FNV-1a over w0..w5 + avalanche, linear probing,
 * lm_slots a power of two.  lm_order <= 6; start_id = the id of "<s>" (< lm_vocab, the
 * LM's word count); dict_cols = the label count dict_next was built for (must equal c);
 * an arc past dict_states is treated as leading to the post-space state; c <= 64.
 * Same outputs and workspace as ds2_ctc_beam_decode (scores include the LM terms). */
ds2_status_t ds2_ctc_beam_decode_lm(const float* probs, int n, int t_max, int c, int64_t stride_n,
                                    int64_t stride_t, const int* sizes, int blank, int beam_width,
                                    int cutoff_top_n, double cutoff_prob, int top_paths,
                                    int space_id, int lm_order, int start_id, int lm_vocab,
                                    double alpha, double beta, const int* dict_next,
                                    const void* dict_mask, const int* dict_word, int dict_states,
                                    int dict_cols, const int* lm_table, int64_t lm_slots,
                                    int* out_ids, int* out_offsets, int* out_lens,
                                    float* out_scores, void* ws, size_t ws_bytes,
                                    ds2_stream_t stream);

/* The same two searches over a stream: probabilities arrive in chunks and the beam is
 * carried between calls, so a feed costs its own frames only and the result after the last
 * chunk is the whole-utterance search's, whatever the partition (same kernel, one more
 * template parameter).
 * State: one opaque device buffer of ds2_ctc_beam_stream_state_size(n, max_frames,
 * beam_width) bytes, 256-byte aligned, owned by the caller: per stream the beam (entries,
 * scores, LM dictionary state and history) and its prefix trie, sized once for max_frames
 * frames (36 bytes per node, max_frames * beam_width + 1 nodes per stream).  The size is 0
 * for arguments no state exists for (n, max_frames or beam_width < 1, beam_width > 128).
 * ds2_ctc_beam_stream_init resets all n streams to the empty prefix (start of an utterance).
 * ds2_ctc_beam_stream_feed[_lm]: the arguments of ds2_ctc_beam_decode[_lm] with t_chunk =
 * this chunk's frame count (>= 0), then
 *   sizes       device int32 [n]: this chunk's valid frames per stream (clamped to
 *               [0, t_chunk]; NULL = all); a stream with 0 valid frames keeps its state as
 *               it is, bit for bit
 *   max_frames, beam_width: as given to the size query and to init (a record initialised
 *               for other values is not advanced and reports -1 in out_frames)
 *   t_done      frames fed by earlier calls since init (the caller's count: no call
 *               synchronises); t_done + t_chunk > max_frames is DS2_INVALID_VALUE, and no
 *               stream consumes a frame past max_frames whatever t_done says
 *   out_ids / out_offsets [n][top_paths][out_cap], out_lens / out_scores [n][top_paths]:
 *               the current top_paths prefixes of every stream in full, offsets counted
 *               from the stream's first frame; with the LM the scores include the last
 *               partial word, which the carried state does not.  All four NULL: no read-out
 *               (any other mix is DS2_INVALID_VALUE); out_cap >= t_done + t_chunk
 *   out_frames  device int32 [n] or NULL: frames each stream has consumed so far
 * beam_width, c limits and DS2_UNSUPPORTED_SHAPE as for ds2_ctc_beam_decode.
 * DS2_INVALID_VALUE, before anything is launched, also for a NULL or misaligned state and a
 * state_bytes below the size query.  n == 0, or t_chunk == 0 without read-out, is DS2_OK and
 * launches nothing.  A stream whose beam emptied stays empty.  Feeds of one state must be
 * ordered (one stream, or events); the LM and cutoffs must not change within an utterance. */
size_t ds2_ctc_beam_stream_state_size(int n, int max_frames, int beam_width);
ds2_status_t ds2_ctc_beam_stream_init(void* state, size_t state_bytes, int n, int max_frames,
                                      int beam_width, ds2_stream_t stream);
ds2_status_t ds2_ctc_beam_stream_feed(const float* probs, int n, int t_chunk, int c,
                                      int64_t stride_n, int64_t stride_t, const int* sizes,
                                      int blank, int beam_width, int cutoff_top_n,
                                      double cutoff_prob, int top_paths, int max_frames,
                                      int t_done, int out_cap, int* out_ids, int* out_offsets,
                                      int* out_lens, float* out_scores, int* out_frames,
                                      void* state, size_t state_bytes, ds2_stream_t stream);
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
                                         void* state, size_t state_bytes, ds2_stream_t stream);

/* bf16 GEMM on bf16 operands (BASELINE cfg4's bf16 MFMA RNN GEMMs; csrc/bgemm.hip):
 * C[m x n] (fp32, ldc) = alpha * A . B^T + beta * C + bias, A [m][lda] and B [n][ldb] bf16
 * (raw 16-bit words, k-contiguous), fp32 accumulation.  A and B 16-B aligned, k, lda, ldb
 * multiples of 8, each operand < 2 GiB, else DS2_UNSUPPORTED_SHAPE.  Workspace for the
 * split-K tail: ds2_bgemm_workspace_size (NULL / too small: no split).
 * ds2_cvt_bf16: fp32 [rows][ld_src] -> bf16 (round to nearest even) as [rows][ld_dst], or
 * with transpose != 0 as [cols][ld_dst] (the k-contiguous copy of an m- or n-contiguous
 * operand).                                                                    */
size_t ds2_bgemm_workspace_size(int m, int n, int k);
ds2_status_t ds2_bgemm_nt(int m, int n, int k, float alpha, const void* a, int64_t lda,
                          const void* b, int64_t ldb, float beta, float* c, int64_t ldc,
                          const float* bias, void* ws, size_t ws_bytes, ds2_stream_t stream);
ds2_status_t ds2_cvt_bf16(const float* src, int rows, int cols, int64_t ld_src, void* dst,
                          int64_t ld_dst, int transpose, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Vanilla tanh RNN recurrence (supported_rnns['rnn'] = nn.RNN, model.py:15; csrc/rnn.hip):
 * h_t = tanh(xproj_t + b_hh + W_hh h_{t-1}) over packed lengths, xproj / h_all / dy / dgates
 * laid out as for ds2_gru_fwd / ds2_gru_bwd with one gate ([T][N][D][H]); dgates = the
 * gradient wrt the pre-activation (= dgx = dgh of the GEMMs).  One launch per step.      */
ds2_status_t ds2_rnn_fwd(int t_max, int n, int h, int num_dirs, const float* xproj,
                         const float* w_hh_f, const float* w_hh_r, const float* b_hh_f,
                         const float* b_hh_r, const int* lens, float* h_all,
                         ds2_stream_t stream);
ds2_status_t ds2_rnn_bwd(int t_max, int n, int h, int num_dirs, const float* dy, int dy_dirs,
                         const float* w_hh_f, const float* w_hh_r, const float* h_all,
                         const int* lens, float* dgates, ds2_stream_t stream);
/* The same recurrences on the GRU's persistent machinery (one launch per layer and pass: the
 * one-gate fp16x3 instantiations of the GRU kernels, csrc/gru_split.hip), with the per-step
 * kernels above as the fallback for shapes they decline (H % 16 != 0, a grid past the CUs)
 * and DS2_RNN_PERSISTENT=0.  err_out as for ds2_gru_fwd.  col_amax (nullable): [D H] column
 * maxima of |dgates| as float bits (ds2_amax's format) for the fp16x3 weight-gradient GEMMs;
 * D H must then be a multiple of 4 as for ds2_amax (DS2_UNSUPPORTED_SHAPE otherwise, nothing
 * launched: pass NULL).
 * ds2_rnn_bwd_grid: workgroups the persistent backward holds at once (0: per-step kernels). */
size_t ds2_rnn_fwd_workspace_size(int n, int h, int num_dirs);
ds2_status_t ds2_rnn_fwd_ws(int t_max, int n, int h, int num_dirs, const float* xproj,
                            const float* w_hh_f, const float* w_hh_r, const float* b_hh_f,
                            const float* b_hh_r, const int* lens, float* h_all, unsigned* err_out,
                            void* ws, size_t ws_bytes, ds2_stream_t stream);
size_t ds2_rnn_bwd_workspace_size(int n, int h, int num_dirs);
int ds2_rnn_bwd_grid(int n, int h, int num_dirs);
ds2_status_t ds2_rnn_bwd_ws(int t_max, int n, int h, int num_dirs, const float* dy, int dy_dirs,
                            const float* w_hh_f, const float* w_hh_r, const float* h_all,
                            const int* lens, float* dgates, unsigned* col_amax, unsigned* err_out,
                            void* ws, size_t ws_bytes, ds2_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Data-parallel gradient exchange over RCCL (SURVEY §8b allreduce_bucket /
 * ds2_comm_t; replaces DistributedDataParallel's bucketed all-reduce, train.py:947-951).
 * Rank 0 makes an id (ds2_comm_id_bytes() bytes), the caller carries it to every
 * rank (torch.distributed or a file), each rank creates its communicator on its GPU;
 * ds2_allreduce_bucket sums one contiguous fp32 bucket in place across the ranks,
 * enqueued on `stream` (no averaging: the caller scales once after the last bucket).
 * RCCL is loaded at run time (librccl.so.1); DS2_RCCL_ERROR with ds2_last_error()
 * when it is missing or a collective fails.                                      */
typedef struct ds2_comm* ds2_comm_t;
size_t ds2_comm_id_bytes(void);
ds2_status_t ds2_comm_get_unique_id(void* id_out);
ds2_status_t ds2_comm_init(ds2_comm_t* comm, const void* id, int nranks, int rank, int device);
ds2_status_t ds2_allreduce_bucket(ds2_comm_t comm, float* bucket, int64_t count,
                                  ds2_stream_t stream);
ds2_status_t ds2_comm_destroy(ds2_comm_t comm);

/* ------------------------------------------------------------------------ */
/* Training-step tail (ref train.py:595-632): clip_grad_norm_(max_norm) then
 * SGD(momentum, nesterov) on flat fp32 buffers.  The global L2 norm is reduced
 * on device (fp64), nothing returns to the host.  If skip_flag != NULL and
 * *skip_flag != 0 the step is skipped (NaN guard, train.py:625-630).          */
size_t ds2_optim_workspace_size(int64_t numel);
ds2_status_t ds2_grad_norm(const float* grads, int64_t numel, float* out_norm, void* ws,
                           size_t ws_bytes, ds2_stream_t stream);
ds2_status_t ds2_clip_sgd_nesterov(float* params, const float* grads, float* momentum_buf,
                                   int64_t numel, float lr, float momentum, float max_norm,
                                   const float* norm, const int* skip_flag,
                                   ds2_stream_t stream);
/* The same with torch.optim.SGD's weight_decay: the update runs on
 * g' = g*coef + weight_decay*p (clipping scales .grad before step() adds the decay). */
ds2_status_t ds2_clip_sgd_nesterov_wd(float* params, const float* grads, float* momentum_buf,
                                      int64_t numel, float lr, float momentum,
                                      float weight_decay, float max_norm, const float* norm,
                                      const int* skip_flag, ds2_stream_t stream);
/* clip_grad_norm_(max_norm) then torch.optim.Adam (amsgrad, maximize and decoupled decay
 * off; ref train.py:150-152) in one pass over flat fp32 buffers.  With t = *step + 1:
 *   g' = g*coef (+ weight_decay*p);  m += (1-beta1)(g'-m);  v = beta2 v + (1-beta2) g'^2;
 *   p -= lr/(1-beta1^t) * m / (sqrt(v)/sqrt(1-beta2^t) + eps)
 * The hyper-parameters are doubles, as torch holds them: 1-beta, the bias corrections and
 * lr/(1-beta1^t) are formed in double and rounded to float once.  step is a device word,
 * the count of steps taken: read by the update and advanced by a one-thread kernel behind
 * it on the same stream (no host sync, no race).  A skipped step (skip_flag as above)
 * leaves params, both moments and *step unchanged.                                  */
ds2_status_t ds2_clip_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                           int64_t numel, double lr, double beta1, double beta2, double eps,
                           double weight_decay, float max_norm, const float* norm, int* step,
                           const int* skip_flag, ds2_stream_t stream);
/* *flag = 1 if any x is NaN (flag must be zeroed by the caller first);
 * if zero_nans, NaNs are replaced by 0 in place (train.py:595-598); mask
 * (nullable, one byte per element) records where the NaNs were.              */
ds2_status_t ds2_nan_guard(float* x, int64_t numel, int zero_nans, int* flag,
                           unsigned char* mask, ds2_stream_t stream);
/* Gradient of that in-place zeroing (autograd's index_put, train.py:598):
 * x[i] = 0 where mask[i]; a no-op when flag is non-NULL and *flag == 0.      */
ds2_status_t ds2_zero_masked(float* x, const unsigned char* mask, int64_t numel, const int* flag,
                             ds2_stream_t stream);
/* x[i] *= *scalar (device scalar, e.g. autograd's grad_output). */
ds2_status_t ds2_scale_by_device_scalar(float* x, int64_t numel, const float* scalar,
                                        ds2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DS2HIP_H */
