"""CPU: the C ABI and the host-side contract of the beam search over a stream
(ds2_ctc_beam_stream_*, ds2amd.decoder.StreamingBeamCTCDecoder).  Nothing is launched: every
call here must return from its argument checks."""
import os
import re

import pytest

import torch
from ds2amd import _lib, ops
from ds2amd.decoder import BeamCTCDecoder, StreamingBeamCTCDecoder
from oracle import ds2_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ds2hip.h")
NEW = ["ds2_ctc_beam_stream_state_size", "ds2_ctc_beam_stream_init", "ds2_ctc_beam_stream_feed",
       "ds2_ctc_beam_stream_feed_lm"]
OK, INVALID, UNSUPPORTED = 0, 1, 2


def test_symbols_exported_and_arity_matches_header():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text)
        assert m, f"{name} is not declared in ds2hip.h"
        assert len(_lib._PROTOS[name][1]) == m.group(1).count(",") + 1, name
    for name in ("ops.ctc_beam_stream_state", "ops.ctc_beam_stream_feed_raw",
                 "ops.ctc_beam_stream_feed_lm_raw"):
        assert callable(getattr(ops, name.split(".")[1]))
    # the feeds take their non-LM / LM siblings' arguments plus the same stream arguments
    extra = len(_lib._PROTOS["ds2_ctc_beam_stream_feed"][1]) - len(_lib._PROTOS["ds2_ctc_beam_decode"][1])
    extra_lm = (len(_lib._PROTOS["ds2_ctc_beam_stream_feed_lm"][1])
                - len(_lib._PROTOS["ds2_ctc_beam_decode_lm"][1]))
    assert extra == extra_lm == 4   # max_frames, t_done, out_cap, out_frames


def test_state_size():
    size = lambda *a: _lib.size("ds2_ctc_beam_stream_state_size", *a)
    for bad in [(0, 100, 10), (-1, 100, 10), (1, 0, 10), (1, -5, 10), (1, 100, 0), (1, 100, 129),
                (1, 2 ** 30, 100)]:
        assert size(*bad) == 0, bad
    base = size(2, 100, 10)
    assert base % 256 == 0
    assert size(3, 100, 10) > base
    assert size(2, 101, 10) > base
    assert size(2, 100, 11) > base
    # the trie dominates: 36 bytes per node, max_frames * beam_width + 1 nodes per stream
    assert size(1, 3000, 100) >= 36 * (3000 * 100 + 1)
    assert size(1, 3000, 100) <= 36 * (3000 * 100 + 1) + 64 * 1024
    # and it is the whole-utterance workspace for max_frames plus the beam records
    assert size(4, 500, 128) > _lib.size("ds2_ctc_beam_workspace_size", 4, 500, 128)


# probs, n, t_chunk, c, stride_n, stride_t, sizes, blank, beam, top_n, cutoff, top_paths,
# max_frames, t_done, out_cap, ids, offsets, lens, scores, frames, state, state_bytes, stream.
# Pointers are fake (never dereferenced on the host); 256 is an aligned one.
def _feed_args(**kw):
    a = dict(probs=256, n=2, t_chunk=8, c=30, stride_n=240, stride_t=30, sizes=None, blank=0,
             beam=10, top_n=40, cutoff=1.0, top_paths=1, max_frames=100, t_done=0, out_cap=8,
             ids=256, offs=256, lens=256, scores=256, frames=None, state=256, state_bytes=1 << 30,
             stream=None)
    a.update(kw)
    return list(a.values())


def _feed_lm_args(**kw):
    a = _feed_args(**kw)
    # space, order, start, vocab, alpha, beta, dict_next, dict_mask, dict_word, states, cols,
    # table, slots
    lm = [29, 3, 0, 9, 0.8, 1.0, 256, 256, 256, 5, a[3], 256, 8]
    return a[:12] + lm + a[12:]


@pytest.mark.parametrize("lm", [False, True])
def test_feed_rejects_without_launch(lm):
    lib = _lib.load()
    fn = lib.ds2_ctc_beam_stream_feed_lm if lm else lib.ds2_ctc_beam_stream_feed
    mk = _feed_lm_args if lm else _feed_args
    need = _lib.size("ds2_ctc_beam_stream_state_size", 2, 100, 10)
    # the instance limits of the whole-utterance entry
    assert fn(*mk(beam=129, top_paths=1)) == UNSUPPORTED
    assert fn(*mk(c=65, stride_t=65)) == (INVALID if lm else UNSUPPORTED)   # the LM entry: c <= 64
    assert fn(*mk(beam=33, c=65, stride_t=65)) == (INVALID if lm else UNSUPPORTED)
    # capacity: t_done + t_chunk > max_frames
    assert fn(*mk(t_done=93, out_cap=200)) == INVALID
    assert fn(*mk(t_done=92, out_cap=99)) == INVALID        # out_cap below t_done + t_chunk
    assert fn(*mk(out_cap=7)) == INVALID
    assert fn(*mk(t_chunk=101, out_cap=200)) == INVALID
    # the state: short, NULL, not 256-byte aligned
    assert fn(*mk(state_bytes=need - 1)) == INVALID
    assert fn(*mk(state=None)) == INVALID
    assert fn(*mk(state=256 + 128)) == INVALID
    # read-out pointers: all four or none
    assert fn(*mk(scores=None)) == INVALID
    assert fn(*mk(ids=None, offs=None)) == INVALID
    # the whole-utterance entry's own argument checks
    for bad in [dict(n=-1), dict(t_chunk=-1), dict(blank=30), dict(top_paths=0),
                dict(top_paths=11), dict(top_n=0), dict(t_done=-1), dict(max_frames=0)]:
        assert fn(*mk(**bad)) == INVALID, bad
    # nothing to do: DS2_OK, and nothing launched (the fake pointers would fault)
    assert fn(*mk(n=0)) == OK
    assert fn(*mk(t_chunk=0, ids=None, offs=None, lens=None, scores=None)) == OK


def test_init_rejects_without_launch():
    lib = _lib.load()
    need = _lib.size("ds2_ctc_beam_stream_state_size", 2, 100, 10)
    assert lib.ds2_ctc_beam_stream_init(256, need - 1, 2, 100, 10, None) == INVALID
    assert lib.ds2_ctc_beam_stream_init(None, need, 2, 100, 10, None) == INVALID
    assert lib.ds2_ctc_beam_stream_init(128, need, 2, 100, 10, None) == INVALID
    assert lib.ds2_ctc_beam_stream_init(256, 1 << 40, 0, 100, 10, None) == INVALID
    assert lib.ds2_ctc_beam_stream_init(256, 1 << 40, 2, 0, 10, None) == INVALID
    assert lib.ds2_ctc_beam_stream_init(256, 1 << 40, 2, 100, 129, None) == INVALID
    with pytest.raises(_lib.Ds2Error):
        ops.ctc_beam_stream_state(0, 100, 10, "cpu")


def test_decoder_constructor_limits():
    assert issubclass(StreamingBeamCTCDecoder, BeamCTCDecoder)
    d = StreamingBeamCTCDecoder(orc.LABELS)
    assert (d.beam_width, d.max_frames, d.top_paths, d.frames_fed) == (100, 3000, 1, 0)
    d = StreamingBeamCTCDecoder(orc.LABELS, beam_width=128, max_frames=7, top_paths=128)
    assert (d.beam_width, d.max_frames, d.top_paths) == (128, 7, 128)
    with pytest.raises(ValueError):
        StreamingBeamCTCDecoder(orc.LABELS, beam_width=129)
    with pytest.raises(ValueError):
        StreamingBeamCTCDecoder(orc.LABELS + "0123456789" * 4)
    with pytest.raises(ValueError):
        StreamingBeamCTCDecoder(orc.LABELS, max_frames=0)
    with pytest.raises(ValueError):
        StreamingBeamCTCDecoder(orc.LABELS, beam_width=10, top_paths=11)
    with pytest.raises(ValueError):
        StreamingBeamCTCDecoder(orc.LABELS, top_paths=0)


def test_feed_needs_the_gpu_and_counts_frames_on_the_host(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(_lib, "size", lambda *a: calls.append(a) or 0)
    c = len(orc.LABELS)
    d = StreamingBeamCTCDecoder(orc.LABELS, beam_width=10, max_frames=20)
    with pytest.raises(RuntimeError):
        d.feed(torch.full((2, 5, c), 1.0 / c))
    with pytest.raises(RuntimeError):
        d.finish()                               # nothing fed: no stream count, no device
    with pytest.raises(ValueError):
        d.feed(torch.full((2, 21, c), 1.0 / c))  # past max_frames: the host count decides
    with pytest.raises(ValueError):
        d.feed(torch.full((2, 5, c + 1), 1.0 / (c + 1)))
    d.frames_fed = 18                            # as after 18 fed frames
    with pytest.raises(ValueError):
        d.feed(torch.full((2, 3, c), 1.0 / c))
    with pytest.raises(RuntimeError):
        d.feed(torch.full((2, 2, c), 1.0 / c))   # fits; a CPU tensor all the same
    assert d.frames_fed == 18
    assert calls == []                           # every error came before any library call
