"""GPU: ds2_pcm_decode (ops.pcm_decode) against ds2amd.data_loader.load_audio_norm on the
same wav files, bit for bit (torch.equal), and parse_batch on raw Waves against parse_batch
on the float arrays of the same files.  The output is NaN before the kernel runs, so a
padding column it does not write shows.  Every wav is written here, 1 s at the most."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from ds2amd import _lib, ops
from ds2amd.audio_aug import Wave, pack_raw
from ds2amd.data_loader import SpectrogramParser, load_audio_norm, load_audio_raw

pytestmark = pytest.mark.gpu

CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
COUNTS = [1, 63, 64, 65, 255, 256, 257, 4097, 16000]


def _write(tmp_path, name, data, sr=16000):
    path = os.path.join(str(tmp_path), name + ".wav")
    wavfile.write(path, sr, data)
    return path


def _decode(dev, files, out_stride=None):
    """files: [(path, selector)] -> (ops.pcm_decode rows over NaN-filled memory, the
    load_audio_norm arrays)."""
    waves = [load_audio_raw(p, c)[0] for p, c in files]
    assert all(w.raw is not None for w in waves)
    _, _, total = pack_raw(waves)
    buf = np.zeros(total, dtype=np.uint8)
    desc, hdr, total = pack_raw(waves, buf)
    packed = torch.from_numpy(buf[hdr:].view(np.int16).copy()).to(dev)
    stride = out_stride or max(w.n_in for w in waves)
    out = torch.full((len(waves), stride), float('nan'), device=dev)
    assert ops.pcm_decode(packed, desc, stride, out=out) is out
    return out.cpu(), [load_audio_norm(p, c)[0] for p, c in files], desc


def _check(out, refs, stride):
    for b, ref in enumerate(refs):
        ref = torch.from_numpy(np.ascontiguousarray(ref.reshape(-1)))
        assert ref.dtype == torch.float32
        assert torch.equal(out[b, :ref.numel()], ref), f"row {b}"
        assert torch.equal(out[b, ref.numel():], torch.zeros(stride - ref.numel())), f"pad {b}"


def _rand(rng, *shape):
    return rng.integers(-32768, 32768, size=shape).astype(np.int16)


def test_mono_lengths_and_alignment(dev, tmp_path):
    """The frame counts in packed order: an odd count leaves the next file 2-byte aligned
    only; 4097 and 16000 take several blocks per utterance."""
    rng = np.random.default_rng(1)
    files = [(_write(tmp_path, f"m{n}", _rand(rng, n)), -1) for n in COUNTS]
    files.append((_write(tmp_path, "col", _rand(rng, 257, 1)), -1))     # [n, 1]
    out, refs, desc = _decode(dev, files)
    assert [int(v) % 2 for v in desc[:, 0]] == [0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    _check(out, refs, 16000)


@pytest.mark.parametrize("ch", [2, 3, 8])
def test_channels_and_selectors(dev, tmp_path, ch):
    """Interleaved channels, selector -1 (float32 mean as ndarray.mean(axis=1) sums it:
    sequential below 8 channels, pairwise at 8), 0 and last, over the same frame counts."""
    rng = np.random.default_rng(ch)
    files = []
    for n in COUNTS[:8]:
        p = _write(tmp_path, f"c{ch}_{n}", _rand(rng, n, ch))
        files += [(p, -1), (p, 0), (p, ch - 1)]
    out, refs, _ = _decode(dev, files)
    _check(out, refs, 4097)


def test_peak_edge_cases(dev, tmp_path):
    rng = np.random.default_rng(7)
    low = rng.integers(-30000, 30000, size=(4097, 2)).astype(np.int16)
    last = low.copy()
    last[-1, 1] = 32001                              # the peak is the very last sample
    neg = rng.integers(-30000, 30000, size=300).astype(np.int16)
    neg[17] = -32767
    pos = neg.copy()
    pos[17] = 32767
    data = {
        "zero": np.zeros(65, np.int16),              # abs_max 0: not scaled, no NaN
        "wrap": np.array([-32768, 100, -7], np.int16),   # abs_max 100 (|-32768| wraps)
        "allmin": np.full(63, -32768, np.int16),     # abs_max -32768: not scaled
        "allmin2": np.full((63, 2), -32768, np.int16),
        "neg": neg, "pos": pos, "last": last,
        "zero2": np.zeros((5, 3), np.int16),
    }
    files = [(_write(tmp_path, k, v), -1) for k, v in data.items()]
    out, refs, _ = _decode(dev, files)
    assert refs[1].tolist() == [np.float32(-327.68), 1.0, np.float32(-0.07)]
    assert float(refs[2][0]) == -32768.0
    _check(out, refs, 4097)
    assert not torch.isnan(out).any()


def test_out_stride_beyond_longest_row(dev, tmp_path):
    rng = np.random.default_rng(9)
    files = [(_write(tmp_path, f"s{n}", _rand(rng, n)), -1) for n in (65, 1, 1500)]
    out, refs, _ = _decode(dev, files, out_stride=1500 + 1031)
    _check(out, refs, 1500 + 1031)


def test_argument_checks(dev):
    """Rejected before any launch; n == 0 is DS2_OK."""
    lib = _lib.load()
    packed = torch.zeros(64, dtype=torch.int16, device=dev)
    assert ops.pcm_decode(packed, np.zeros((0, 4), np.int64), 16).shape == (0, 16)
    assert lib.ds2_pcm_decode(None, 0, None, None, 0, None, 0, None, 0, None) == 0
    assert lib.ds2_pcm_decode(None, 0, None, None, -1, None, 0, None, 0, None) == 1
    for row, stride in [((0, 8, 0, -1), 8),        # ch 0
                        ((0, 2, 9, -1), 8),        # ch 9
                        ((0, 8, 2, 2), 8),         # selector == ch
                        ((0, 8, 2, -2), 8),        # selector < -1
                        ((0, 8, 1, -1), 7),        # out_stride too small
                        ((0, -1, 1, -1), 8),       # negative frames
                        ((-2, 8, 1, -1), 8),       # negative offset
                        ((60, 8, 1, -1), 8),       # past the buffer
                        ((0, 8, 1, -1), -8)]:      # negative stride
        with pytest.raises(_lib.Ds2Error, match="DS2_INVALID_VALUE"):
            ops.pcm_decode(packed, np.array([row], np.int64), stride)
    torch.cuda.synchronize()


@pytest.mark.parametrize("switch", [None, "0"])
def test_parse_batch_raw_equals_float(dev, tmp_path, monkeypatch, switch):
    """parse_batch on raw Waves == parse_batch on the float arrays of the same files, with
    one 8 kHz file under the 16 kHz config (a RESAMPLE round: apply_waves), and without (the
    plain upload); the same with DS2_PCM_DECODE=0."""
    if switch is None:
        monkeypatch.delenv("DS2_PCM_DECODE", raising=False)
    else:
        monkeypatch.setenv("DS2_PCM_DECODE", switch)
    from ds2amd.audio_aug import RESAMPLE, heavy_length
    rng = np.random.default_rng(3)
    files = [(_write(tmp_path, "a", _rand(rng, 4097)), 16000),
             (_write(tmp_path, "b", _rand(rng, 1601, 2)), 16000),
             (_write(tmp_path, "c", _rand(rng, 3999)), 16000),
             (_write(tmp_path, "d", _rand(rng, 2001)), 8000)]
    parser = SpectrogramParser(CONF, normalize='max_frame', device=dev)

    def waves(raw, subset):
        out = []
        for path, sr in subset:
            w = load_audio_raw(path)[0] if raw else Wave(load_audio_norm(path)[0])
            assert (w.raw is not None) == raw
            if sr != 16000:
                w.record(RESAMPLE, a=sr, b=16000)
                w.length = heavy_length(RESAMPLE, sr, 16000, 0.0, w.length)
            out.append(w)
        return out

    for subset in (files, files[:3]):
        got, gf = parser.parse_batch(waves(True, subset))
        ref, rf = parser.parse_batch(waves(False, subset))
        assert torch.equal(gf, rf)
        assert torch.equal(got, ref)
    # the float arrays themselves (no Wave): today's call
    ref, _ = parser.parse_batch([load_audio_norm(p)[0] for p, _ in files[:3]])
    assert torch.equal(got, ref)
