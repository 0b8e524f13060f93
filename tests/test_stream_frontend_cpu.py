"""CPU: the streaming front-end's host side -- the count of final frames against np.pad(reflect)
framing, the partitions the GPU tests run, the causal 'max_frame' restatement and its
sensitivity, the constructor's refusals, and the entry points' argument checks that end before
any launch."""
import numpy as np
import pytest

from ds2amd import _lib, ops
from ds2amd.streaming import StreamingFrontend

import frontend_common as fc
import stream_frontend_common as sc

P = 0x1000          # a non-NULL, 256-byte aligned "pointer": every call here ends before a launch


@pytest.mark.parametrize("n_fft,hop", sc.GEOMETRIES)
def test_final_frame_count_is_np_pad_framing(n_fft, hop):
    """For a = 1 .. 3 n_fft: the frames of the prefix that read the samples the whole utterance's
    frames read are ops.stft_stream_frames(0, a, False), which is the issue's rule; at the end
    the count is librosa's."""
    longer = sc.padded_index(5 * n_fft, n_fft, hop)
    for a in range(1, 3 * n_fft + 1):
        want = sc.final_frames_brute(a, n_fft, hop, longer)
        assert sc.final_frames_rule(a, n_fft, hop) == want, a
        assert ops.stft_stream_frames(0, a, False, n_fft, hop) == want, a
        assert ops.stft_stream_frames(0, a, True, n_fft, hop) == fc.frames_of(a, n_fft, hop), a
    assert ops.stft_stream_frames(0, 0, False, n_fft, hop) == 0
    assert ops.stft_stream_frames(0, 0, True, n_fft, hop) == 0


def test_counts_of_a_feed():
    assert ops.stft_stream_frames(0, 160, False, 320, 160) == 0
    assert ops.stft_stream_frames(0, 161, False, 320, 160) == 1
    assert ops.stft_stream_frames(0, 320, False, 320, 160) == 2
    assert ops.stft_stream_frames(161, 320, False, 320, 160) == 1
    assert ops.stft_stream_frames(320, 320, True, 320, 160) == 1      # finish: 3 frames in all
    assert ops.stft_stream_frames(100, 100, True, 320, 160) == 1      # n <= pad: all at finish
    for n_fft, hop in sc.GEOMETRIES:
        assert ops.stft_stream_frames(0, sc.samples_for_frames(5, n_fft, hop), False, n_fft, hop) == 5
        assert ops.stft_stream_frames(0, sc.samples_for_frames(5, n_fft, hop) - 1, False, n_fft,
                                      hop) == 4
    with pytest.raises(ValueError):
        ops.stft_stream_frames(5, 4, False, 320, 160)


@pytest.mark.parametrize("n_fft,hop", sc.GPU_GEOMETRIES)
def test_partitions_reach_the_edges_they_claim(n_fft, hop):
    for n in sc.LENGTHS:
        parts = sc.partitions(n, n_fft, hop)
        assert ("single" in parts) == (n <= 321)
        for name, sizes in parts.items():
            assert sum(sizes) == n and min(sizes) >= 0, (n, name)
    parts = sc.partitions(6400, n_fft, hop)
    per_feed = {}
    for name, sizes in parts.items():
        ends = np.cumsum(sizes)
        per_feed[name] = [ops.stft_stream_frames(e - s, e, False, n_fft, hop)
                          for s, e in zip(sizes, ends)]
    assert per_feed["f789"][:4] == [1, 7, 8, 9]
    assert per_feed["fssf"][:5] == [1, sc.SSF - 1, sc.SSF, sc.SSF + 1, 2 * sc.SSF + 1]
    assert per_feed["zero"][:6] == [0, 1, 0, 1, 0, 0]
    assert 0 in sc.partitions(6400, n_fft, hop)["mixed"]


def test_causal_restatement_and_its_sensitivity():
    """The definition by hand on three frames; an offset per call instead of per frame and a
    1-indexed denominator both move the result by far more than the bound."""
    n_fft, hop = 320, 160
    y = fc.signal("ramp", 1280, 3, hop)
    r = sc.causal_refs("ramp", 1280, 3, n_fft, hop)
    m = r.val.mean(axis=0)
    assert r.ref.shape == (161, 9)
    assert np.allclose(r.off[:3], [m[0], (m[0] + m[1]) / 2, (m[0] + m[1] + m[2]) / 3], rtol=1e-14)
    assert np.array_equal(r.ref, r.val - r.off[None, :])
    o0, w = 7.0, 4.0
    rp = sc.causal_refs("ramp", 1280, 3, n_fft, hop, (o0, w))
    assert np.allclose(rp.off[:2], [(w * o0 + m[0]) / (w + 1), (w * o0 + m[0] + m[1]) / (w + 2)],
                       rtol=1e-14)
    assert 0 < r.e_ref < 1e-4 and r.bound < 1e-4
    for wrong, kw in (("per_call", dict(calls=[1, 3, 5])), ("one_indexed", {})):
        bad = sc.causal_ref64(y, n_fft, hop, wrong=wrong, **kw)[0]
        assert np.abs(bad - r.ref).max() > 100 * r.bound, wrong
    # silence: val = 0, so the output is minus the offset, which the prior alone sets
    s = sc.causal_refs("silence", 640, 0, n_fft, hop, (o0, w))
    assert np.array_equal(s.val, np.zeros_like(s.val))
    assert np.allclose(s.ref[0], [-w * o0 / (w + t + 1) for t in range(5)], rtol=1e-14)


CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')


@pytest.mark.parametrize("kw,what", [
    (dict(normalize='mean'), "whole utterance"),
    (dict(normalize='norm'), "whole utterance"),
    (dict(normalize='frame'), "whole utterance"),
    (dict(normalize='max'), "modes"),
    (dict(normalize='none', offset=1.0), "offset="),
    (dict(normalize='none', prior=(1.0, 2.0)), "prior="),
    (dict(offset=1.0, prior=(1.0, 2.0)), "prior="),
    (dict(n_streams=0), "n_streams"),
    (dict(device='cpu'), "GPU only"),
])
def test_constructor_refusals(kw, what):
    with pytest.raises(ValueError, match=what):
        StreamingFrontend(CONF, **kw)


def test_constructor_refuses_geometries_that_cannot_stream():
    # 8 kHz: n_fft 160, 81 bins -- the mirror-fill reads ahead
    with pytest.raises(ValueError, match="mirror-fill"):
        StreamingFrontend(dict(CONF, sample_rate=8000))
    with pytest.raises(ValueError, match="mirror-fill"):
        StreamingFrontend(dict(CONF, window_size=0.019))          # n_fft 304: 153 bins
    with pytest.raises(ValueError, match="n_fft // 2"):
        StreamingFrontend(dict(CONF, window_size=0.032))          # n_fft 512: 257 bins
    with pytest.raises(ValueError, match="n_fft <= 1024"):
        StreamingFrontend(dict(CONF, sample_rate=44100, window_size=0.025))


def _feed(chunk=P, dtype=0, n=2, samples=320, stride=320, scale=1.0, done=0, last=0, n_fft=320,
          hop=160, window=P, normalize=1, fixed=None, out=P, k=2, state=P, state_bytes=None,
          ws=P, ws_bytes=None):
    if state_bytes is None:
        state_bytes = _lib.size("ds2_stft_stream_state_size", max(n, 1), n_fft, hop)
    if ws_bytes is None:
        ws_bytes = _lib.size("ds2_stft_stream_workspace_size", max(n, 1), max(k, 1))
    return _lib.load().ds2_stft_stream_feed(chunk, dtype, n, samples, stride, scale, done, last,
                                            n_fft, hop, window, normalize, fixed, out, k, None,
                                            None, state, state_bytes, ws, ws_bytes, None)


def test_sizes_and_status_codes_before_any_launch():
    size = lambda *a: _lib.size("ds2_stft_stream_state_size", *a)
    # per stream: a 64-byte head, pad + 1 and n_fft - 1 float32 samples, rounded up to 256
    assert size(1, 320, 160) == -(-(64 + 4 * (161 + 319)) // 256) * 256
    assert size(3, 400, 160) == 3 * (-(-(64 + 4 * (201 + 399)) // 256) * 256)
    assert size(0, 320, 160) == size(1, 318, 160) == size(1, 512, 160) == size(1, 320, 0) == 0
    assert _lib.size("ds2_stft_stream_workspace_size", 3, 5) == 256
    assert _lib.size("ds2_stft_stream_workspace_size", 3, 0) == 0
    init = _lib.load().ds2_stft_stream_init
    need = size(2, 320, 160)
    assert init(None, need, 2, 320, 160, None, 0.0, None) == fc.INVALID_VALUE
    assert init(P + 4, need, 2, 320, 160, None, 0.0, None) == fc.INVALID_VALUE
    assert init(P, need - 1, 2, 320, 160, None, 0.0, None) == fc.INVALID_VALUE
    assert init(P, need, 2, 320, 160, None, -1.0, None) == fc.INVALID_VALUE
    assert init(P, need, 2, 160, 80, None, 0.0, None) == fc.UNSUPPORTED_SHAPE
    assert init(P, need, 2, 512, 80, None, 0.0, None) == fc.UNSUPPORTED_SHAPE
    assert init(P, need, 2, 2048, 80, None, 0.0, None) == fc.INVALID_VALUE
    # feed: k is the host's count for (done, samples, last)
    assert _feed(k=1) == _feed(k=3) == fc.INVALID_VALUE
    assert _feed(samples=160, stride=160, k=1) == fc.INVALID_VALUE            # no frame yet
    assert _feed(done=320, samples=0, last=1, k=0) == fc.INVALID_VALUE        # finish: 1 frame
    assert _feed(samples=-1) == _feed(done=-1) == _feed(k=-1) == fc.INVALID_VALUE
    assert _feed(dtype=2) == _feed(last=2) == _feed(normalize=2) == fc.INVALID_VALUE
    assert _feed(normalize=0, fixed=P) == fc.INVALID_VALUE
    assert _feed(stride=319) == fc.INVALID_VALUE
    assert _feed(n=-1) == fc.INVALID_VALUE
    assert _feed(done=2 ** 31 - 400, samples=320, k=2) == fc.INVALID_VALUE
    assert _feed(n_fft=160, hop=80, k=4) == fc.UNSUPPORTED_SHAPE
    assert _feed(state=None) == _feed(state=P + 16) == fc.INVALID_VALUE
    assert _feed(state_bytes=need - 1) == fc.INVALID_VALUE
    assert _feed(chunk=None) == _feed(window=None) == _feed(out=None) == fc.INVALID_VALUE
    assert _feed(ws=None) == _feed(ws_bytes=255) == fc.WORKSPACE_TOO_SMALL
    # nothing to do: no streams, or no samples and the utterance stays open
    assert _feed(n=0) == fc.OK
    assert _feed(samples=0, stride=0, done=320, k=0, chunk=None, state=None) == fc.OK
