"""CPU: the tables, references and bounds of the audio front-end contract tests (frontend_common,
run on the GPU by test_gpu_frontend_contract.py), every status code of the four entry points and
three workspace queries they cover, and the host's refusals.  The tables reach the block, length
and reflect edges their rows claim, by the kernels' constants restated in frontend_common; the
float64 STFT reference agrees with the oracle and loses that agreement under each of eight
deliberate mistakes, by far more than the bound the device is held to; every refusal returns
before any HIP call, so the pointers handed over here are never dereferenced (0x1000 stands for
"not NULL")."""
import math

import numpy as np
import pytest
import torch

from ds2amd import _lib, ops
from ds2amd import audio_aug as aa
from oracle import ds2_oracle as orc
from oracle import librosa_effects as le

import frontend_common as fc
from frontend_common import (INVALID_VALUE, OK, STFT_CASES, UNSUPPORTED_SHAPE,
                             WORKSPACE_TOO_SMALL)

P = 0x1000      # a non-NULL pointer no call below reaches far enough to use


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------
# the tables

def test_frame_counts_are_the_oracles_and_differ_from_the_old_formula_where_claimed():
    """ops.stft_frames is np.pad + framing's count; 1 + n // hop is one too many exactly when
    n_fft is odd and hop divides n (the issue's three examples included)."""
    for sr, n, want, old in ((22050, 2200, 10, 11), (15999, 1113, 7, 8), (16050, 1600, 10, 11)):
        n_fft, hop = int(sr * (0.02 + 1e-8)), int(sr * (0.01 + 1e-8))
        assert orc.stft_magnitude(np.zeros(n, np.float32), sr).shape[1] == want
        assert ops.stft_frames(n, n_fft, hop) == want and 1 + n // hop == old
    for case, c in STFT_CASES.items():
        for (n, _, _), t in zip(c.rows, fc.case_frames(case)):
            assert ops.stft_frames(n, c.n_fft, c.hop) == t
            assert (1 + n // c.hop != t) == (c.n_fft % 2 == 1 and n % c.hop == 0), (case, n)
    odd = [(case, n) for case, c in STFT_CASES.items() for n, _, _ in c.rows
           if c.n_fft % 2 and n % c.hop == 0]
    assert ("f441", 220) in odd and ("f441", 2200) in odd and ("r319", 159) in odd


def test_the_stft_table_reaches_the_edges_its_rows_claim():
    frames = {case: fc.case_frames(case) for case in STFT_CASES}
    bins = {case: c.n_fft // 2 + 1 for case, c in STFT_CASES.items()}
    # paths: fused at F >= 161 (cut to 161 rows above it), remap below
    assert bins["f320"] == fc.ROWS and bins["f441"] == 221 and bins["f510"] == fc.MAX_BINS
    assert [bins[c] for c in ("r160", "r319", "r220", "r80", "r2")] == [81, 160, 111, 41, 2]
    assert STFT_CASES["r319"].n_fft % 2 == 1 and bins["r319"] == fc.ROWS - 1
    # fused: T on, one below and one above a block of SF frames, and two blocks and a frame
    assert frames["f320"] == [1, 1, 1, 2, 2, fc.SF - 1, fc.SF, fc.SF + 1, 2 * fc.SF + 1]
    # reflect folds of the 160-sample pad: many, twice, exactly once (pad == n - 1)
    fold = lambda n, pad: math.inf if n == 1 else _cdiv(pad, n - 1)
    lens = [n for n, _, _ in STFT_CASES["f320"].rows]
    assert [fold(n, 160) for n in lens[:5]] == [math.inf, 160, 2, 2, 1] and lens[4] - 1 == 160
    # the capped subtract grid: 814 frames fill 512 blocks, 815 need a 513th
    assert fc.sub_blocks(814) == fc.SUB_CAP and fc.sub_blocks(815) == fc.SUB_CAP + 1
    assert frames["f320_hop16"] == [816, 3] and fc.sub_blocks(816) > fc.SUB_CAP
    assert all(fc.sub_blocks(max(t) + STFT_CASES[c].extra_frames) <= fc.SUB_CAP
               for c, t in frames.items() if c != "f320_hop16")
    assert frames["f441"] == [1, 1, 1, 10, 10, 11]
    # remap: T = 1, 3, 4, 5 around the 4-column block, two of the lengths multiples of hop
    for case in ("r160", "r319", "r220", "r80"):
        c = STFT_CASES[case]
        assert frames[case] == [1, fc.REMAP_COLS - 1, fc.REMAP_COLS, fc.REMAP_COLS + 1]
        assert sum(n % c.hop == 0 for n, _, _ in c.rows) >= 2
    # F = 41: 161 T values span more frames than there are, so rows come from later frames and,
    # past F T values, from the zero fill
    assert all(fc.ROWS * t > bins["r80"] * t for t in frames["r80"])
    assert STFT_CASES["r2"].rows[0][0] == 5 and frames["r2"] == [6]
    # one call per path with room in max_frames and max_samples
    for case in ("f320", "r160"):
        assert STFT_CASES[case].extra_frames == 3 and STFT_CASES[case].extra_samples > 0
    # every kind of signal on both paths; the defect rows are not silent
    for cases in (("f320", "f441"), ("r160", "r319", "r220", "r80")):
        assert {k for c in cases for _, k, _ in STFT_CASES[c].rows} == set(fc.KINDS)
    kinds = {n: k for n, k, _ in STFT_CASES["f441"].rows}
    assert kinds[220] != "silence" and kinds[2200] != "silence"


def test_the_mask_rows_are_the_hand_written_ones():
    for case in ("f320_masks", "r160_masks"):
        c = STFT_CASES[case]
        assert fc.case_frames(case) == [fc.MASK_T] * 8 and len(c.masks) == 8
        m = np.array(c.masks)
        assert (m[0, 0] == m[0, 1]) and (m[0, 4] == m[0, 5])                     # empty
        assert m[1, :4].tolist() == [0, 1, 160, 161]
        assert m[2, 4:8].tolist() == [0, 1, fc.MASK_T - 1, fc.MASK_T]
        assert m[3, 5] == fc.MASK_T + 1
        assert m[4, 0] < m[4, 2] < m[4, 1] < m[4, 3] and m[4, 4] < m[4, 6] < m[4, 5] < m[4, 7]
        assert m[5:, 8].tolist() == [0, 81, 161]
        # f_cut 0: all masked; 'norm' is 0 / 0 in the float64 reference and in the oracle's chain
        for mode in range(5):
            r = fc.stft_refs(case, mode)[5]
            assert np.isnan(r.ref).all() and np.isnan(r.r32).all() if mode == 3 else not r.ref.any()


def test_the_stretch_table_reaches_the_edges_its_rows_claim():
    plans = [ops.stretch_plan(n, r) for n, r, _ in fc.STRETCH_ROWS]
    short = {(n, r): p for (n, r, _), p in zip(fc.STRETCH_ROWS, plans)}
    assert short[(3072, 0.2)][1:] == (35, 34)            # the ISTFT's length-limited frame count
    # 3 / 0.1 is 30.0 in float64: np.arange gives 30 steps (not 31), the ISTFT uses 24 of them
    assert short[(1024, 0.1)][1:] == (30, 24) and math.ceil(3 / 0.1) == 30
    assert all(p[2] == p[1] for k, p in short.items() if k[1] >= 0.25)
    # steps whose second column is the padding after the last input frame ...
    n_in = lambda n: 1 + n // fc.FX_HOP
    assert int(29 * 0.1) + 1 == n_in(1024) and int(3 * 3.0) + 1 == n_in(5000)
    # ... and one whose columns both are: 9 / 0.072 rounds to 125.00000000000001, a 126th step
    assert short[(4096, 0.072)][1:] == (126, 116) and int(125 * 0.072) == n_in(4096) == 9
    lens = [n for n, _, _ in fc.STRETCH_ROWS]
    assert {1, 2, 511, 512, 513, 1023, 1024, 1025} <= set(lens)          # one frame, two, three
    for (e, f, noise), p, (n, r, _) in zip(fc.stretch_refs(), plans, fc.STRETCH_ROWS):
        print(f"FRONTEND stretch len {n} rate {r}: noise {noise:.3e} of the peak")
        assert len(e) == len(f) == p[0] and np.isfinite(e).all() and np.isfinite(f).all()
        # up to 2.6e-3 on the short rows; the 126 steps at rate 0.072 accumulate 1.3e-2
        assert e.dtype == np.float32 and np.abs(e).max() > 0 and noise <= (2.6e-3 if r > 0.072 else 2e-2)


def test_the_resample_table_reaches_the_edges_its_rows_claim():
    assert {fc.WING - 1, fc.WING, fc.WING + 1, 1, 2} <= set(fc.RESAMPLE_LENS)
    ratios = [b / a for a, b in fc.RESAMPLE_PAIRS]
    assert ratios == [2.0, 0.5, 16000 / 22050, 1.0, 17959.5 / 16000, 16000 / 44100]
    for name in ("s256", "s257"):
        stride, rows = fc.RESAMPLE_BATCHES[name]
        assert len(rows) == 42
        zero = [r for r in rows if r.valid == 0]
        assert any(r.n == 1 and r.pair == (16000, 8000) for r in zero)      # n_valid = 0 ...
        assert le.resample(np.ones(1, np.float32), 16000, 8000).shape == (1,)   # ... out_len 1
        assert any(0 < r.out_len < r.valid for r in rows) and any(r.out_len > r.valid for r in rows)
        assert all(min(r.valid, r.out_len) <= stride for r in rows)
        for r, e in zip(rows, fc.resample_refs(name)):
            assert len(e) == r.valid == int(r.n * (float(r.pair[1]) / r.pair[0]))
    stride, rows = fc.RESAMPLE_BATCHES["rows65"]
    assert len(rows) == fc.TREG_BLOCK + 1 and all(r.n == 2 for r in rows)


def test_the_wave_table_reaches_the_edges_its_rows_claim():
    rows, noise = fc.wave_rows(), fc.wave_noise()
    kinds = [[k for k, _, _, _ in recs] for _, recs in rows]
    assert [fc.S, fc.D, fc.N, fc.S] in kinds and [fc.D, fc.D] in kinds and [] in kinds
    assert kinds.count([fc.N]) == 2
    used = [a for _, recs in rows for k, a, _, _ in recs if k == fc.N]
    assert len(used) > len(set(used)) > 1                              # shared and distinct rows
    assert {len(y) for y, _ in rows} == {1, 63, fc.WAV_T - 1, fc.WAV_T, fc.WAV_T + 1, 2 * fc.WAV_T + 1}
    shifts = [(a, b) for _, recs in rows for k, a, b, _ in recs if k == fc.S]
    assert (0, 0) in shifts and any(a == b > 0 for a, b in shifts) and any(a == 0 < b for a, b in shifts)
    assert max(len(recs) for _, recs in rows) == fc.WAVE_MAX_OPS
    neg, last = rows[6][0], rows[7][0]
    assert (neg < 0).all() and np.argmax(last) == len(last) - 1
    ref = fc.wave_ref(*rows[6], noise)
    assert (ref == neg.max()).all()                # np.clip with min > max: the maximum everywhere
    np.testing.assert_array_equal(fc.wave_ref(*rows[5], noise), rows[5][0])
    for y, recs in rows:
        final, cap = fc.wave_lengths(y, recs)
        assert fc.wave_ref(y, recs, noise).shape == (final,) and cap <= noise.shape[1]


# ------------------------------------------------------------------------------------------
# the STFT references

SR_OF = {"f320": (16000, 0.01), "f320_hop16": (16000, 0.001), "f441": (22050, 0.01),
         "f510": (25500, 0.01), "r160": (8000, 0.01), "r319": (15950, 0.01), "r220": (11000, 0.01),
         "r80": (4000, 0.01), "r2": (100, 0.01)}


@pytest.mark.parametrize("case", list(SR_OF))
def test_the_float32_restatement_is_the_oracles_spectrogram(case):
    """stft_ref32 takes (n_fft, hop); orc.spectrogram derives them from a sample rate.  Bit-equal
    at a rate that gives the case's geometry, in every mode."""
    c = STFT_CASES[case]
    sr, stride = SR_OF[case]
    assert (int(sr * (0.02 + 1e-8)), int(sr * (stride + 1e-8))) == (c.n_fft, c.hop)
    for mode, norm in enumerate(fc.NORMS):
        for y, r in zip(fc.case_signals(case), fc.stft_refs(case, mode)):
            with np.errstate(invalid="ignore", divide="ignore"):
                want = orc.spectrogram(y, sr, window_stride=stride, normalize=norm).numpy()
            assert np.array_equal(r.r32.astype(np.float32), want, equal_nan=True), (case, norm)


@pytest.mark.parametrize("case", list(STFT_CASES))
def test_the_float64_reference_agrees_with_the_oracle(case):
    """Same frame count, same NaNs (silence under 'norm' only), and a distance e_ref of float32
    rounding size: a few ulps of the values before the offset is subtracted (log1p(2^20 |X|)
    reaches ~20), times the 1 / mean(std) of 'norm'."""
    c = STFT_CASES[case]
    for mode in range(5):
        for (n, kind, _), r in zip(c.rows, fc.stft_refs(case, mode)):
            print(f"FRONTEND {case} mode {mode} n {n} {kind}: e_ref {r.e_ref:.3e}  bound {r.bound:.3e}")
            assert r.ref.shape == r.r32.shape == (fc.ROWS, fc.frames_of(n, c.n_fft, c.hop))
            assert fc.same_nans(r.ref, r.r32)
            masked_out = c.masks is not None and c.masks[c.rows.index((n, kind, _))][8] == 0
            assert np.isnan(r.ref).any() == (mode == 3 and (kind == "silence" or masked_out))
            assert r.e_ref <= (2e-4 if mode == 3 else 4e-6)
            if kind == "silence" or masked_out:
                assert r.e_ref == 0


MISTAKES = {
    # mistake: ((case, mode, row) ...) on which it must show
    "frames": (("f441", 0, 4), ("f441", 2, 2), ("r319", 0, 2)),
    "edge_pad": (("f320", 2, 1), ("r2", 0, 0), ("f441", 0, 2)),
    "np_reflect": (("r80", 1, 1), ("f320_masks", 4, 2), ("f320", 4, 6)),
    "row_major": (("r160", 2, 2), ("r319", 0, 3)),
    "mirror": (("r80", 1, 2), ("r160", 0, 3)),
    "biased_std": (("f320", 3, 3), ("r160", 3, 2)),
    "mask_hi": (("r160_masks", 0, 2), ("f320_masks", 1, 2), ("f320_masks", 0, 6)),
    "gain": (("f320", 1, 0), ("r160_masks", 1, 4)),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_each_deliberate_mistake_moves_the_reference_far_past_the_bound(mistake):
    """The evidence that the GPU comparison can fail: the reference with one mistake is more
    than 10 bounds away from the reference, on every row named for it."""
    for case, mode, row in MISTAKES[mistake]:
        c = STFT_CASES[case]
        r = fc.stft_refs(case, mode)[row]
        mask = c.masks[row] if c.masks else fc.NO_MASK
        bad = fc.stft_ref64(fc.case_signals(case)[row], c.n_fft, c.hop, mode, mask, wrong=mistake)
        ratio = fc.max_diff(bad, r.ref) / r.bound
        print(f"FRONTEND sensitivity {mistake}: {case} mode {mode} row {row} (n {c.rows[row][0]}, "
              f"{c.rows[row][1]}): {ratio:.3g} bounds")
        assert np.isfinite(ratio) and ratio > 10


def test_no_mistake_is_a_no_op_switch():
    """wrong=None is the reference, and an unknown mode of the oracle still raises."""
    y = fc.case_signals("r160")[1]
    assert np.array_equal(fc.stft_ref64(y, 160, 80, 2), fc.stft_ref64(y, 160, 80, 2, wrong=None))
    with pytest.raises(Exception):
        orc.normalize_audio(np.zeros((161, 2), np.float32), "bogus")


# ------------------------------------------------------------------------------------------
# status codes, in the order the entry points check

def _stft(pcm=P, ns=P, batch=2, max_samples=400, n_fft=320, hop=160, window=P, normalize=0,
          taps=None, radius=0, masks=None, out=P, max_frames=3, ws=P, ws_bytes=None, masked=True):
    lib = _lib.load()
    if ws_bytes is None:
        ws_bytes = _lib.size("ds2_stft_workspace_size", max(batch, 0), max(max_frames, 0), n_fft)
    head = (pcm, ns, batch, max_samples, n_fft, hop, window, normalize, taps, radius)
    tail = (out, max_frames, ws, ws_bytes, None)
    if masked:
        return lib.ds2_stft_logmag_masked(*head, masks, *tail)
    return lib.ds2_stft_logmag(*head, *tail)


@pytest.mark.parametrize("masked", [True, False])
def test_stft_status_codes(masked):
    call = lambda **kw: _stft(masked=masked, ws=None, ws_bytes=0, **kw)    # ends at the workspace
    assert call() == WORKSPACE_TOO_SMALL
    assert call(batch=-1) == INVALID_VALUE
    for n_fft in (1, 0, -2, fc.MAX_NFFT + 1):
        assert call(n_fft=n_fft) == INVALID_VALUE
    assert call(hop=0) == INVALID_VALUE and call(max_frames=0) == INVALID_VALUE
    # thread = bin: F = 257 and 513 are refused, 256 is the widest
    assert call(n_fft=512) == UNSUPPORTED_SHAPE and call(n_fft=fc.MAX_NFFT) == UNSUPPORTED_SHAPE
    assert call(n_fft=510) == WORKSPACE_TOO_SMALL and call(n_fft=511) == WORKSPACE_TOO_SMALL
    assert call(n_fft=2, hop=1) == WORKSPACE_TOO_SMALL
    # a bad size comes before the unsupported shape, that before the mode
    assert call(n_fft=512, hop=0) == INVALID_VALUE
    assert call(n_fft=512, normalize=5) == UNSUPPORTED_SHAPE
    assert call(normalize=-1) == INVALID_VALUE and call(normalize=5) == INVALID_VALUE
    for mode in (1, 4):                                  # the smoothing modes need their taps
        assert call(normalize=mode) == INVALID_VALUE
        assert call(normalize=mode, taps=P, radius=-1) == INVALID_VALUE
        assert call(normalize=mode, taps=P, radius=0) == WORKSPACE_TOO_SMALL
    for mode in (0, 2, 3):
        assert call(normalize=mode) == WORKSPACE_TOO_SMALL
    # batch 0 is done before the workspace is looked at, and after the arguments are
    assert call(batch=0, pcm=None, ns=None, out=None) == OK
    assert call(batch=0, normalize=7) == INVALID_VALUE
    need = _lib.size("ds2_stft_workspace_size", 2, 3, 320)
    assert _stft(masked=masked, ws=None, ws_bytes=need) == WORKSPACE_TOO_SMALL
    assert _stft(masked=masked, ws=P, ws_bytes=need - 1) == WORKSPACE_TOO_SMALL


def test_stft_workspace_size():
    """Two float rows of max_frames and two floats per utterance; below 161 bins also the raw
    magnitudes, frame-major."""
    base = lambda b, t: 2 * b * t * 4 + 2 * b * 4 + 512
    for n_fft in (320, 441, 510):
        assert _lib.size("ds2_stft_workspace_size", 3, 17, n_fft) == base(3, 17)
    for n_fft in (2, 80, 160, 220, 319):
        f = n_fft // 2 + 1
        assert _lib.size("ds2_stft_workspace_size", 3, 17, n_fft) == base(3, 17) + 3 * 17 * f * 4 + 256
    assert _lib.size("ds2_stft_workspace_size", 0, 17, 320) == 512


def test_time_stretch_status_codes():
    need = _lib.size("ds2_time_stretch_workspace_size", 2, 3, 4)
    al = lambda v: (v + 255) // 256 * 256
    bins = fc.FX_N // 2 + 1
    assert need == al(2 * 3 * bins * 8) + al(2 * 4 * bins * 8) + al(2 * 4 * fc.FX_N * 8) + 256
    assert _lib.size("ds2_time_stretch_workspace_size", 0, 3, 4) == 256
    assert _lib.size("ds2_time_stretch_workspace_size", -1, 3, 4) == 256

    def call(x=P, x_stride=2000, lens=P, n=2, rate=P, of=P, uf=P, ol=P, win=P, out=P,
             out_stride=2000, max_in=3, max_out=4, ws=None, ws_bytes=0):
        return _lib.load().ds2_time_stretch(x, x_stride, lens, n, rate, of, uf, ol, win, out,
                                            out_stride, max_in, max_out, ws, ws_bytes, None)
    assert call() == WORKSPACE_TOO_SMALL
    for k in ("n", "x_stride", "out_stride", "max_in", "max_out"):
        assert call(**{k: -1}) == INVALID_VALUE, k
    assert call(n=0, x=None, lens=None, rate=None, of=None, uf=None, ol=None, win=None, out=None) == OK
    assert call(n=0, x_stride=-1) == INVALID_VALUE           # the sizes come before the empty batch
    for k in ("x", "lens", "rate", "of", "uf", "ol", "win", "out"):
        assert call(**{k: None}, ws=P, ws_bytes=need) == INVALID_VALUE, k
    assert call(ws=None, ws_bytes=need) == WORKSPACE_TOO_SMALL
    assert call(ws=P, ws_bytes=need - 1) == WORKSPACE_TOO_SMALL


def test_resample_status_codes():
    al = lambda v: (v + 255) // 256 * 256
    assert _lib.size("ds2_resample_workspace_size", 3, 257) == al(3 * 257 * 8) + 256
    assert _lib.size("ds2_resample_workspace_size", 0, 257) == 256
    assert _lib.size("ds2_resample_workspace_size", 3, 0) == 256
    need = _lib.size("ds2_resample_workspace_size", 2, 100)

    def call(x=P, x_stride=100, lens=P, n=2, ratio=P, nv=P, win=P, nwin=32769, table=512, out=P,
             out_stride=100, ws=None, ws_bytes=0):
        return _lib.load().ds2_resample(x, x_stride, lens, n, ratio, nv, win, nwin, table, out,
                                        out_stride, ws, ws_bytes, None)
    assert call() == WORKSPACE_TOO_SMALL
    for k in ("n", "x_stride", "out_stride"):
        assert call(**{k: -1}) == INVALID_VALUE, k
    assert call(nwin=1) == INVALID_VALUE and call(nwin=2) == WORKSPACE_TOO_SMALL
    assert call(table=0) == INVALID_VALUE and call(table=1) == WORKSPACE_TOO_SMALL
    empty = dict(x=None, lens=None, ratio=None, nv=None, win=None, out=None)
    assert call(n=0, **empty) == OK and call(out_stride=0, **empty) == OK
    assert call(n=0, nwin=1) == INVALID_VALUE
    for k in ("x", "lens", "ratio", "nv", "win", "out"):
        assert call(**{k: None}, ws=P, ws_bytes=need) == INVALID_VALUE, k
    assert call(ws=None, ws_bytes=need) == WORKSPACE_TOO_SMALL
    assert call(ws=P, ws_bytes=need - 1) == WORKSPACE_TOO_SMALL


def test_wave_aug_status_codes():
    assert _lib.size("ds2_wave_aug_workspace_size", 3, 100) == 2 * 3 * 100 * 4 + 256
    assert _lib.size("ds2_wave_aug_workspace_size", 0, 100) == 256
    assert _lib.size("ds2_wave_aug_workspace_size", 3, 0) == 256
    need = _lib.size("ds2_wave_aug_workspace_size", 2, 100)

    def call(x=P, in_stride=100, il=P, n=2, op_i=P, op_f=P, max_ops=4, noise=None, ns=0, out=P,
             out_stride=100, ol=P, cap=100, err=P, ws=None, ws_bytes=0):
        return _lib.load().ds2_wave_aug(x, in_stride, il, n, op_i, op_f, max_ops, noise, ns, out,
                                        out_stride, ol, cap, err, ws, ws_bytes, None)
    assert call() == WORKSPACE_TOO_SMALL                     # noise may be NULL
    for k in ("n", "max_ops", "in_stride", "out_stride", "cap"):
        assert call(**{k: -1}) == INVALID_VALUE, k
    assert call(n=0, x=None, il=None, op_i=None, op_f=None, out=None, ol=None, err=None) == OK
    assert call(n=0, cap=-1) == INVALID_VALUE
    for k in ("x", "il", "out", "ol", "err", "op_i", "op_f"):
        assert call(**{k: None}, ws=P, ws_bytes=need) == INVALID_VALUE, k
    # no records, no record arrays
    assert call(max_ops=0, op_i=None, op_f=None) == WORKSPACE_TOO_SMALL
    assert call(ws=None, ws_bytes=need) == WORKSPACE_TOO_SMALL
    assert call(ws=P, ws_bytes=need - 1) == WORKSPACE_TOO_SMALL


# ------------------------------------------------------------------------------------------
# the host's refusals: ValueError before any device work, so CPU tensors get that far

def test_a_zero_length_utterance_is_refused_on_the_host():
    from ds2amd.data_loader import SpectrogramParser
    parser = SpectrogramParser(dict(sample_rate=16000, window_size=0.02, window_stride=0.01),
                               normalize="max_frame", device="cpu")
    for batch in ([np.zeros(0, np.float32)], [np.ones(5, np.float32), np.zeros(0, np.float32)],
                  [aa.Wave(np.zeros(0, np.float32))]):
        with pytest.raises(ValueError, match="no samples"):
            parser.parse_batch(batch)
    with pytest.raises(ValueError):           # what the reference does: np.pad on an empty axis
        orc.spectrogram(np.zeros(0, np.float32))
    for n in (0, -1):
        with pytest.raises(ValueError, match="no frames"):
            ops.stft_frames(n, 320, 160)
    assert ops.stft_frames(1, 320, 160) == 1 == orc.stft_magnitude(np.ones(1, np.float32)).shape[1]


def test_time_stretch_refuses_what_librosa_has_no_answer_for():
    x = torch.zeros(2, 8)
    for lens, rates in (([4, 0], [1.0, 1.0]), ([4, -3], [1.0, 1.0]), ([4, 4], [1.0, 0.0]),
                        ([4, 4], [-0.5, 1.0]), ([4, 4], [1.0, float("nan")])):
        with pytest.raises(ValueError, match="time_stretch"):
            ops.time_stretch(x, lens, rates)
    with pytest.raises(ValueError):
        le.time_stretch(np.ones(4, np.float32), 0.0)
    with pytest.raises(_lib.Ds2Error):        # valid rows get as far as the device-tensor check
        ops.time_stretch(x, [4, 4], [1.0, 1.0])


def test_resample_refuses_a_ratio_whose_table_step_is_zero():
    x = torch.zeros(2, 8)
    assert int(min(1.0, 1 / 512) * 512) == 1 and int(min(1.0, 0.0019) * 512) == 0
    for ratios in ([1.0, 0.0], [-2.0, 1.0], [1.0, 0.0019], [float("nan"), 1.0]):
        with pytest.raises(ValueError, match="resample"):
            ops.resample(x, [4, 4], ratios)
    with pytest.raises(_lib.Ds2Error):
        ops.resample(x, [4, 4], [1.0, 1 / 512])
