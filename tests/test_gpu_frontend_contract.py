"""GPU: the audio front-end kernels (csrc/stft.hip, csrc/effects.hip, csrc/wave.hip's
ds2_wave_aug) on every row of frontend_common's tables against its float64 references and
bounds.  The entry points are called directly: out is NaN before the launch, inputs have NaN past
every row's samples, the workspace is the query's bytes between canaries.  What the tables reach
and why the bounds can fail is test_frontend_contract_cpu.py's part."""
import numpy as np
import pytest
import torch

from ds2amd import _lib, ops
from oracle import ds2_oracle as orc

import frontend_common as fc
from frontend_common import STFT_CASES

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# STFT

def _check_stft(case, mode, got, rows=None):
    """got [B, 161, max_frames] against the case's references: within the bound on each row's
    frames (NaN exactly where the reference has it), exact zeros after them."""
    c = STFT_CASES[case]
    refs = fc.stft_refs(case, mode)
    worst = 0.0
    for b, i in enumerate(range(len(c.rows)) if rows is None else rows):
        r = refs[i]
        t = r.ref.shape[1]
        body, pad = got[b, :, :t].astype(np.float64), got[b, :, t:]
        assert not pad.any() and not np.isnan(pad).any(), f"{case} mode {mode} row {i}: padding frames not zero"
        assert fc.same_nans(body, r.ref), f"{case} mode {mode} row {i}: NaN where the reference has none (or none where it has)"
        err = fc.max_diff(body, r.ref)
        ratio = err / r.bound
        worst = max(worst, ratio)
        print(f"FRONTEND stft {case} mode {mode} row {i} (n {c.rows[i][0]}, {c.rows[i][1]}): "
              f"err {err:.3e}  e_ref {r.e_ref:.3e}  device/bound {ratio:.3f}")
    assert worst <= 1, f"{case} mode {mode}: {worst:.3f} x the bound 4 e_ref + 1 ulp"


@pytest.mark.parametrize("mode", range(5))
@pytest.mark.parametrize("case", list(STFT_CASES))
def test_stft_table_vs_float64(dev, case, mode):
    _check_stft(case, mode, fc.run_stft(case, mode, dev))


@pytest.mark.parametrize("case", ["f320", "f441", "r160", "r319", "f320_masks", "r160_masks"])
def test_stft_row_alone_equals_row_in_the_batch(dev, case):
    """The first, a middle and the last row alone (their own max_frames and max_samples): the
    bits they have inside the ragged batch."""
    n = len(STFT_CASES[case].rows)
    for mode in (1, 3):
        full = fc.run_stft(case, mode, dev)
        for i in (0, n // 2, n - 1):
            one = fc.run_stft(case, mode, dev, rows=[i])
            t = one.shape[2] - STFT_CASES[case].extra_frames
            assert np.array_equal(one[0, :, :t], full[i, :, :t], equal_nan=True), (case, mode, i)
            assert not one[0, :, t:].any() and not full[i, :, t:].any()


def test_stft_unmasked_entry_point_is_the_masked_one_without_masks(dev):
    for case in ("f441", "r319"):
        a = fc.run_stft(case, 1, dev, entry="ds2_stft_logmag")
        assert np.array_equal(a, fc.run_stft(case, 1, dev), equal_nan=True)
        _check_stft(case, 1, a)


def test_a_row_without_samples_is_all_zero_and_reads_nothing(dev):
    """n_samples <= 0 (the host refuses it; the kernels must still not divide by T = 0 or index
    pcm): the row is zero in every mode, its neighbour unchanged.  The row's pcm is all NaN."""
    for n_bad in (0, -5):
        for name in ("f320", "r160"):
            c = STFT_CASES[name]
            y = fc.case_signals(name)[3]
            for mode in range(5):
                host = torch.full((2, len(y) + 3), float("nan"))
                host[1, :len(y)] = torch.from_numpy(y)
                pcm = fc.Poisoned(host, dev)
                ns = fc._i32([n_bad, len(y)], dev)
                t = fc.frames_of(len(y), c.n_fft, c.hop)
                out = fc.Poisoned((2, fc.ROWS, t + 1), dev)
                ws = fc.Workspace(_lib.size("ds2_stft_workspace_size", 2, t + 1, c.n_fft), dev)
                win = torch.from_numpy(orc.hamming(c.n_fft)).to(dev)
                taps = None
                if mode in fc.SIGMA:
                    taps = torch.from_numpy(fc.gaussian_taps(fc.SIGMA[mode]).astype(np.float32)).to(dev)
                _lib.call("ds2_stft_logmag", pcm.ptr, ns.ptr, 2, len(y) + 3, c.n_fft, c.hop,
                          win.data_ptr(), mode, None if taps is None else taps.data_ptr(),
                          0 if taps is None else (taps.numel() - 1) // 2, out.ptr, t + 1, ws.ptr,
                          ws.nbytes, None)
                torch.cuda.synchronize()
                got = out.read().numpy()
                assert out.intact() and ws.intact()
                assert not got[0].any() and not np.isnan(got[0]).any(), (name, mode, n_bad)
                r = fc.stft_refs(name, mode)[3]
                assert fc.max_diff(got[1, :, :t].astype(np.float64), r.ref) <= r.bound


@pytest.mark.parametrize("sr,n", [(22050, 2200), (16000, 1), (22050, 220), (15950, 159)])
@pytest.mark.parametrize("norm", ["max_frame", "norm"])
def test_parse_batch_frame_counts_and_spectra_at_the_defect_lengths(dev, sr, n, norm):
    """SpectrogramParser end to end where 1 + n // hop was one frame too many (odd n_fft, hop
    divides n) and where the pad has one sample to reflect: the oracle's frame count, its
    spectrum within the table's kind of bound, zeros after it."""
    from ds2amd.data_loader import SpectrogramParser
    conf = dict(sample_rate=sr, window_size=0.02, window_stride=0.01, window="hamming")
    parser = SpectrogramParser(conf, normalize=norm, device=dev)
    n_fft, hop = int(sr * (0.02 + 1e-8)), int(sr * (0.01 + 1e-8))
    wavs = [fc.signal("ramp", n, 900, hop), fc.signal("ramp", n + 3 * hop + 1, 901, hop)]
    out, frames = parser.parse_batch(wavs, sr)
    for i, y in enumerate(wavs):
        ref = orc.spectrogram(y, sr, normalize=norm).numpy().astype(np.float64)
        ref64 = fc.stft_ref64(y, n_fft, hop, fc.NORMS.index(norm))
        t = ref.shape[1]
        assert int(frames[i]) == t == ops.stft_frames(len(y), n_fft, hop)
        got = out[i, 0].cpu().numpy().astype(np.float64)
        e_ref = fc.max_diff(ref, ref64)
        bound = 4 * e_ref + float(np.spacing(np.float32(np.abs(ref64).max())))
        err = fc.max_diff(got[:, :t], ref64)
        print(f"FRONTEND parse_batch sr {sr} n {len(y)} {norm}: T {t}  err {err:.3e}  e_ref {e_ref:.3e}  "
              f"device/bound {err / bound:.3f}")
        assert err <= bound and fc.max_diff(got[:, :t], ref) <= bound + e_ref
        assert not got[:, t:].any()
    assert int(frames[0]) == (1 + (n - 1) // hop if n_fft % 2 else 1 + n // hop)


# ------------------------------------------------------------------------------------------
# time stretch

def _check_stretch(out, lens, rows):
    refs = fc.stretch_refs()
    bad = []
    for b, i in enumerate(rows):
        e, f, noise = refs[i]
        n, rate, kind = fc.STRETCH_ROWS[i]
        assert lens[b] == len(e)
        got = out[b, :len(e)]
        assert np.isfinite(got).all(), f"stretch row {i}: an output sample was never written"
        assert not out[b, len(e):].any() and not np.isnan(out[b, len(e):]).any()
        err, err64 = fc.rel_diff(got, e), fc.rel_diff(got, f)
        r1, r2 = err / (0.75 * noise + 2e-6), err64 / (1.5 * noise + 2e-6)
        print(f"FRONTEND stretch row {i} (len {n}, rate {rate}, {kind}): noise {noise:.3e}  "
              f"vs restatement {err:.3e} ({r1:.3f} of its bound)  vs float64 {err64:.3e} ({r2:.3f})")
        if r1 > 1 or r2 > 1:
            bad.append((i, r1, r2))
    assert not bad, bad


def test_time_stretch_table_vs_oracle(dev):
    """The ragged batch under test_time_stretch_device_matches_oracle's bound: at most 0.75 noise
    + 2e-6 from the restatement and 1.5 noise + 2e-6 from the float64 chain, noise being the
    restatement's own distance from that chain."""
    out, lens = fc.run_stretch(dev)
    _check_stretch(out, lens, range(len(fc.STRETCH_ROWS)))


def test_time_stretch_row_alone_equals_row_in_the_batch(dev):
    full, lens = fc.run_stretch(dev)
    for i in (0, 4, 10, 11, 12):
        one, l1 = fc.run_stretch(dev, rows=[i])
        assert l1[0] == lens[i] and np.array_equal(one[0, :l1[0]], full[i, :l1[0]]), i


# ------------------------------------------------------------------------------------------
# resample

@pytest.mark.parametrize("batch", list(fc.RESAMPLE_BATCHES))
def test_resample_table_vs_oracle(dev, batch):
    """Within 2 float32 ulps of the restatement on the samples asked for, zero after them, in
    both output strides and past fx_treg_kernel's first block."""
    out = fc.run_resample(batch, dev)
    _, rows = fc.RESAMPLE_BATCHES[batch]
    worst = 0.0
    for i, (r, e) in enumerate(zip(rows, fc.resample_refs(batch))):
        k = min(r.valid, r.out_len)
        got = out[i]
        assert np.isfinite(got).all(), f"{batch} row {i}: an output sample was never written"
        assert not got[k:].any(), f"{batch} row {i}: not zero past n_valid {k}"
        d = np.abs(got[:k].astype(np.float64) - e[:k])
        tol = 2 * np.spacing(np.abs(e[:k]).astype(np.float32)).astype(np.float64) + 1e-12
        if k:
            worst = max(worst, float((d / tol).max()))
    print(f"FRONTEND resample {batch}: worst device/bound {worst:.3f}")
    assert worst <= 1


def test_resample_wrapper_pads_to_out_lens(dev):
    """ops.resample with out_lens: librosa's fix_length (ceil against resampy's floor)."""
    y = fc.signal("ramp", 65, 950, 16)
    out, lens = ops.resample(torch.from_numpy(y)[None].to(dev), [65], [16000 / 22050], out_lens=[48])
    e = fc.le.resample(y, 22050, 16000)
    assert lens == [48] == [len(e)]
    d = np.abs(out[0].cpu().numpy() - e)
    assert (d <= 2 * np.spacing(np.abs(e)) + 1e-12).all() and e[47] == 0 == out[0, 47].item()


# ------------------------------------------------------------------------------------------
# wave aug

def test_wave_aug_chains_vs_replay(dev):
    """Chains of up to four ops through both ping-pong buffers: bit-equal without NOISE, within
    one float32 ulp with it (the device may contract the float64 mix into an FMA)."""
    rows, noise = fc.wave_rows(), fc.wave_noise()
    out, err = fc.run_wave(rows, noise, dev)
    assert err == 0
    for i, (y, recs) in enumerate(rows):
        ref = fc.wave_ref(y, recs, noise)
        got = out[i]
        assert not got[len(ref):].any() and not np.isnan(got[len(ref):]).any(), i
        if any(k == fc.N for k, _, _, _ in recs):
            d = np.abs(got[:len(ref)].astype(np.float64) - ref)
            ratio = float((d / np.spacing(np.abs(ref))).max())
            print(f"FRONTEND wave row {i} (len {len(y)}, {len(recs)} ops): {ratio:.3f} ulp")
            assert ratio <= 1, i
        else:
            assert np.array_equal(got[:len(ref)], ref), i
    # the wrapper, with its own output: the same bits
    op_i, op_f = fc.wave_ops(rows)
    lens = [len(y) for y, _ in rows]
    pcm = torch.zeros(len(rows), max(lens))
    for i, (y, _) in enumerate(rows):
        pcm[i, :len(y)] = torch.from_numpy(y)
    finals = [fc.wave_lengths(y, recs) for y, recs in rows]
    got = ops.wave_aug(pcm.to(dev), torch.tensor(lens, dtype=torch.int32).to(dev),
                       torch.from_numpy(op_i).to(dev), torch.from_numpy(op_f).to(dev),
                       torch.from_numpy(noise).to(dev), [f for f, _ in finals],
                       out.shape[1], max(c for _, c in finals), check=True)
    assert np.array_equal(got.cpu().numpy(), out)


def test_wave_aug_row_alone_equals_row_in_the_batch(dev):
    rows, noise = fc.wave_rows(), fc.wave_noise()
    full, _ = fc.run_wave(rows, noise, dev)
    for i in (0, 2, 8):
        one, err = fc.run_wave([rows[i]], noise, dev)
        n = fc.wave_lengths(*rows[i])[0]
        assert err == 0 and np.array_equal(one[0, :n], full[i, :n]), i


y100 = lambda: fc.signal("ramp", 100, 960)
WAVE_ERRORS = {
    # name: (records, keyword arguments of run_wave, noise table?, the word)
    "shift_above_limit": ([(fc.S, 4, 3, 0.0)], {}, True, fc.ERR_CAP),
    "shift_past_cap": ([(fc.S, 0, 10, 0.0)], dict(cap=105), True, fc.ERR_CAP),
    "kind_9": ([(9, 0, 0, 0.0)], {}, True, fc.ERR_RECORD),
    "out_lens_off_by_one": ([(fc.D, 0, 0, 1.0)], dict(out_lens=[101, 63]), True, fc.ERR_LENGTH),
    "in_lens_above_cap": ([(fc.D, 0, 0, 1.0)], dict(cap=99), True, fc.ERR_CAP),
    "noise_without_table": ([(fc.N, 0, 0, 0.1)], {}, False, fc.ERR_RECORD),
}


@pytest.mark.parametrize("name", list(WAVE_ERRORS))
def test_wave_aug_consistency_word(dev, name):
    """A record that cannot be replayed sets the word and leaves that row of out (and everything
    outside the buffers) unwritten; the good row beside it is replayed.  ops.wave_aug raises."""
    recs, kw, with_noise, word = WAVE_ERRORS[name]
    noise = fc.wave_noise() if with_noise else None
    good = (fc.signal("tone", 63, 961), [(fc.D, 0, 0, 1.01)])
    rows = [(y100(), recs), good]
    if "out_lens" not in kw:
        kw = dict(kw, out_lens=[100 + sum(b for k, _, b, _ in recs if k == fc.S), 63])
    out, err = fc.run_wave(rows, noise, dev, **kw)
    assert err == word
    assert np.isnan(out[0]).all(), "the refused row wrote to out"
    assert np.array_equal(out[1, :63], fc.wave_ref(*good, fc.wave_noise())) and not out[1, 63:].any()
    op_i, op_f = fc.wave_ops(rows)
    pcm = torch.zeros(2, 100)
    pcm[0] = torch.from_numpy(rows[0][0])
    pcm[1, :63] = torch.from_numpy(good[0])
    with pytest.raises(_lib.Ds2Error, match=f"err {word}"):
        ops.wave_aug(pcm.to(dev), torch.tensor([100, 63], dtype=torch.int32).to(dev),
                     torch.from_numpy(op_i).to(dev), torch.from_numpy(op_f).to(dev),
                     None if noise is None else torch.from_numpy(noise).to(dev), kw["out_lens"],
                     128, kw.get("cap", 110), check=True)
