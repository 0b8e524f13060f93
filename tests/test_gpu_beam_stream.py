"""GPU: the prefix beam search over a stream (ds2_ctc_beam_stream_feed[_lm],
ds2amd.decoder.StreamingBeamCTCDecoder).

Whatever the partition of an utterance into chunks, the result after the last chunk is the
whole-utterance search's: ids, char frames and lengths of every returned beam equal those of
ds2_ctc_beam_decode[_lm] and of the CPU oracles (oracle/ctc_beam.py, oracle/ctc_beam_lm.py),
and the scores equal the whole-utterance kernel's bit for bit -- the per-frame body is one
piece of source, and the carried state is copied, never recomputed.  Against the oracles the
scores keep the project's bound, 1e-5 * max(1, |s|).  The generators restate those of
tests/test_gpu_ops.py and tests/test_gpu_beam_wide.py."""
import functools
import os

import numpy as np
import pytest
import torch

from ds2amd import ops
from oracle import ds2_oracle as orc

pytestmark = pytest.mark.gpu

EXTRA = "0123456789абвгдежзийклмнопрстуфхцч"
ARPA = os.path.join(os.path.dirname(__file__), "golden", "tiny_lm.arpa")


def WIDE(n):
    """30 + n labels: '_' blank at 0, ' ' present, so tiny_lm.arpa still applies."""
    return orc.LABELS + EXTRA[:n]


# ---------------------------------------------------------------------------- generators
@functools.lru_cache(maxsize=None)
def _random_case(beam, top_n, cutoff, c):
    """Blank-heavy random softmax (test_ctc_beam_vs_oracle's) and its oracle paths."""
    from oracle import ctc_beam
    g = np.random.default_rng(beam * 10 + top_n)
    n, t = 5, 37
    logits = g.standard_normal((n, t, c)).astype(np.float32) * 3
    logits[:, :, 0] += 1.5
    probs = np.exp(logits - logits.max(-1, keepdims=True))
    probs = (probs / probs.sum(-1, keepdims=True)).astype(np.float32)
    sizes = [37, 30, 1, 0, 22]
    ref = ctc_beam.beam_decode(probs, sizes, beam, cutoff_top_n=top_n, cutoff_prob=cutoff)
    probs.setflags(write=False)
    return probs, sizes, ref


def _spelled(text, g, noise, labels, peak=5.0, blank_bias=1.0):
    frames, prev = [], None
    for ch in text:
        if ch == prev:
            frames.append(0)
        frames += [labels.index(ch), 0]
        prev = ch
    logits = g.standard_normal((len(frames), len(labels))).astype(np.float32) * noise
    logits[:, 0] += blank_bias
    logits[np.arange(len(frames)), frames] += peak
    p = np.exp(logits - logits.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def _batch(ps, c, extra=0):
    t = max(p.shape[0] for p in ps)
    probs = np.full((len(ps) + extra, t, c), 1.0 / c, np.float32)
    for i, p in enumerate(ps):
        probs[i, :p.shape[0]] = p
    return probs


@functools.lru_cache(maxsize=None)
def _lm_case(extra, beam, top_n, alpha, beta, noise):
    """Noisy spelled sentences (test_ctc_beam_lm_vs_oracle's) plus sizes 0 and 1, and the LM
    oracle's paths."""
    from oracle import ctc_beam_lm as obl
    labels = WIDE(extra)
    g = np.random.default_rng(beam * 7 + top_n)
    texts = ["THE CAT SAT ", "I DON'T NO ", "AND THEY SAT ON A HAT", "CATS IN THEN"]
    ps = [_spelled(s, g, noise, labels) for s in texts]
    probs = _batch(ps, len(labels), extra=2)
    sizes = [p.shape[0] for p in ps] + [0, 1]
    ref = obl.beam_decode_lm(probs, sizes, beam, obl.ArpaLM(ARPA), labels, alpha, beta,
                             cutoff_top_n=top_n, cutoff_prob=1.0)
    probs.setflags(write=False)
    return labels, probs, sizes, ref


@functools.lru_cache(maxsize=None)
def _revival_case(extra, beam, top_n, lm):
    """test_wide_beam_trie_revival_vs_oracle's sentences at noise 3.0 and the oracle's paths;
    the oracle must have revived pruned prefixes."""
    from oracle import ctc_beam, ctc_beam_lm as obl
    labels = WIDE(extra)
    g = np.random.default_rng(11)
    ps = [_spelled(s, g, 3.0, labels) for s in ["THE CAT SAT ON A HAT", "I DON'T NO THEN ",
                                                "AND THEY SAT ON A CAT", "CATS IN THEN TOO"]]
    probs = _batch(ps, len(labels))
    sizes = [p.shape[0] for p in ps]
    ctc_beam.STATS["revived"] = 0
    if lm:
        ref = obl.beam_decode_lm(probs, sizes, beam, obl.ArpaLM(ARPA), labels, 0.8, 1.0,
                                 cutoff_top_n=top_n, cutoff_prob=1.0)
    else:
        ref = ctc_beam.beam_decode(probs, sizes, beam, cutoff_top_n=top_n, cutoff_prob=1.0)
    assert ctc_beam.STATS["revived"] > 0
    probs.setflags(write=False)
    return labels, probs, sizes, ref


def _scorer(dev, labels, alpha=0.8, beta=1.0):
    from ds2amd.lm import ArpaScorer
    return ArpaScorer(ARPA, labels, alpha, beta, device=dev)


# ---------------------------------------------------------------------------- runs
def _whole(dev, probs, sizes, beam, top_n, cutoff, scorer=None):
    """The whole-utterance kernel's (ids, offsets, lens, scores) on the CPU."""
    pd = torch.tensor(probs).to(dev)   # a copy: the shared reference inputs stay as they are
    sd = torch.tensor(sizes, dtype=torch.int32).to(dev)
    if scorer is None:
        out = ops.ctc_beam_decode_raw(pd, sd, beam, beam, cutoff_top_n=top_n, cutoff_prob=cutoff)
    else:
        out = ops.ctc_beam_decode_lm_raw(pd, sd, beam, beam, scorer, cutoff_top_n=top_n,
                                         cutoff_prob=cutoff)
    return tuple(x.cpu() for x in out)


def _feed(state, chunk, sd, beam, top_paths, max_frames, done, readout, top_n, cutoff, scorer):
    if scorer is None:
        return ops.ctc_beam_stream_feed_raw(state, chunk, sd, beam, top_paths, max_frames, done,
                                            readout=readout, cutoff_top_n=top_n,
                                            cutoff_prob=cutoff)
    return ops.ctc_beam_stream_feed_lm_raw(state, chunk, sd, beam, top_paths, scorer, max_frames,
                                           done, readout=readout, cutoff_top_n=top_n,
                                           cutoff_prob=cutoff)


def _streamed(dev, probs, sizes, parts, beam, top_n, cutoff, scorer=None, read_each=False,
              state=None):
    """Feed probs [N, T, C] in chunks of `parts` frames (a 0 is an empty chunk), stream n's
    valid frames being its first sizes[n]; the state is sized for exactly T frames.  Returns
    the last read-out on the CPU, the per-chunk read-outs (read_each) and the state."""
    n, t, _ = probs.shape
    assert sum(parts) == t
    pd = torch.tensor(probs).to(dev)
    if state is None:
        state = ops.ctc_beam_stream_state(n, t, beam, dev)
    done, each, out = 0, [], None
    for i, k in enumerate(parts):
        last = i == len(parts) - 1
        sd = torch.tensor([min(max(s - done, 0), k) for s in sizes], dtype=torch.int32).to(dev)
        out = _feed(state, pd[:, done:done + k], sd, beam, beam, t, done, read_each or last,
                    top_n, cutoff, scorer)
        done += k
        assert (out[0] is None) == (not (read_each or last))
        if read_each:
            each.append((done, tuple(x.cpu() for x in out)))
    frames = out[4].cpu().tolist()
    assert frames == [min(s, t) for s in sizes]
    return tuple(x.cpu() for x in out[:4]), each, state


# ---------------------------------------------------------------------------- comparisons
def _same(got, ref, beam, scores=True):
    """_beam_check's assertions."""
    ids, offs, lens, sc = got
    for n, paths in enumerate(ref):
        for p in range(beam):
            if p >= len(paths):
                assert int(lens[n, p]) == 0, (n, p)
                continue
            s, rid, rts = paths[p]
            k = int(lens[n, p])
            assert ids[n, p, :k].tolist() == rid, (n, p)
            assert offs[n, p, :k].tolist() == rts, (n, p)
            if scores:
                assert abs(float(sc[n, p]) - s) <= 1e-5 * max(1.0, abs(s)), (n, p)


def _distinct(got, ref):
    ids, _, lens, _ = got
    for n, paths in enumerate(ref):
        rows = [tuple(ids[n, p, :int(lens[n, p])].tolist()) for p in range(len(paths))]
        assert len(set(rows)) == len(rows), n


def _identical(got, want):
    """Two device searches: lengths, the defined part of ids and char frames (rows (n, p) up
    to lens[n, p]) equal, and the scores the same bits."""
    gi, go, gl, gs = got[:4]
    wi, wo, wl, ws = want[:4]
    assert torch.equal(gl, wl)
    w = min(gi.shape[2], wi.shape[2])
    assert int(gl.max()) <= w
    m = torch.arange(w)[None, None, :] < gl[:, :, None]
    assert torch.equal(gi[:, :, :w] * m, wi[:, :, :w] * m)
    assert torch.equal(go[:, :, :w] * m, wo[:, :, :w] * m)
    assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)), (gs - ws).abs().max()


PARTS37 = {"one": [37], "ones": [1] * 37, "empty-chunks": [0, 5, 0, 32], "primes": [7, 13, 17]}


# ---------------------------------------------------------------------------- 1. partitions
@pytest.mark.parametrize("part", list(PARTS37))
@pytest.mark.parametrize("beam,top_n,cutoff,c", [
    (10, 40, 1.0, 30),     # the small instance
    (100, 40, 1.0, 30),    # the large instance at the reference's default beam
    (100, 40, 1.0, 36),    # the wide instance: the default beam over the Cyrillic label set
    (128, 40, 1.0, 64),    # the wide instance's maxima
    (33, 64, 1.0, 33),     # and its minima
])
def test_partition_invariance(dev, beam, top_n, cutoff, c, part):
    probs, sizes, ref = _random_case(beam, top_n, cutoff, c)
    got, _, _ = _streamed(dev, probs, sizes, PARTS37[part], beam, top_n, cutoff)
    _identical(got, _whole(dev, probs, sizes, beam, top_n, cutoff))
    _same(got, ref, beam)


def test_partition_invariance_with_both_cutoffs(dev):
    beam, top_n, cutoff, c = 100, 10, 0.99, 48
    probs, sizes, ref = _random_case(beam, top_n, cutoff, c)
    got, _, _ = _streamed(dev, probs, sizes, [7, 13, 17], beam, top_n, cutoff)
    _identical(got, _whole(dev, probs, sizes, beam, top_n, cutoff))
    _same(got, ref, beam)


# ---------------------------------------------------------------------------- 2. staging
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("beam,extra,stage", [(8, 0, 128), (40, 0, 128), (40, 10, 64)])
def test_staging_edge(dev, beam, extra, stage, lm):
    """Chunk edges one frame before, on and one frame after the frame at which the
    whole-utterance kernel restages its LDS window of `stage` frames; a stream restages from
    the first frame of every chunk.  T = stage + 3, N = 2 (the second stream ends on the
    stage edge itself)."""
    labels = WIDE(extra)
    t = stage + 3
    g = np.random.default_rng(stage + beam)
    text = "THE CAT SAT ON A HAT AND THEY SAT ON A CAT I DON'T NO THEN CATS IN THEN TOO "
    a = _spelled(text, g, 2.0, labels)[:t]
    b = _spelled(text[20:] + text[:20], g, 2.0, labels)[:stage]
    assert a.shape[0] == t and b.shape[0] == stage
    probs = _batch([a, b], len(labels))
    sizes = [t, stage]
    scorer = _scorer(dev, labels) if lm else None
    whole = _whole(dev, probs, sizes, beam, 40, 1.0, scorer)
    assert int(whole[2][0, 0]) > 20                      # long prefixes
    for parts in ([stage - 1, 1, 3], [stage, 3], [stage + 1, 2]):
        got, _, _ = _streamed(dev, probs, sizes, parts, beam, 40, 1.0, scorer)
        _identical(got, whole)


# ---------------------------------------------------------------------------- 3. LM
# "THE CAT SAT " is spelled T _ H _ E _ ' ' _ C ...: frame 6 is the first space, so these
# chunks end inside a word (3), right before the space frame (6), right after it (7: the next
# chunk starts on the frame after a space, the post-space dictionary state being carried) and
# before the next word's first letter (8)
LM_PARTS = {"word-edges": [3, 3, 1, 1, 5, 0, 9], "ones": None}


@pytest.mark.parametrize("part", list(LM_PARTS))
@pytest.mark.parametrize("extra,beam,top_n,alpha,beta,noise", [
    (0, 8, 40, 0.8, 1.0, 1.5), (0, 100, 40, 0.8, 1.0, 2.0), (6, 100, 40, 0.8, 1.0, 2.0),
    (3, 33, 8, 1.2, 0.5, 3.0)])
def test_lm_partition_invariance(dev, extra, beam, top_n, alpha, beta, noise, part):
    labels, probs, sizes, ref = _lm_case(extra, beam, top_n, alpha, beta, noise)
    t = probs.shape[1]
    parts = LM_PARTS[part]
    parts = [1] * t if parts is None else parts + [t - sum(parts)]
    scorer = _scorer(dev, labels, alpha, beta)
    got, _, _ = _streamed(dev, probs, sizes, parts, beam, top_n, 1.0, scorer)
    _identical(got, _whole(dev, probs, sizes, beam, top_n, 1.0, scorer))
    _same(got, ref, beam)


@pytest.mark.parametrize("lm", [False, True])
def test_trie_revival_across_launches(dev, lm):
    """Chunks of one frame: every revival of a pruned prefix reads trie nodes that an earlier
    launch wrote (children lists, alive counts, char masks)."""
    extra, beam, top_n = 34, 128, 40
    labels, probs, sizes, ref = _revival_case(extra, beam, top_n, lm)
    scorer = _scorer(dev, labels) if lm else None
    got, _, _ = _streamed(dev, probs, sizes, [1] * probs.shape[1], beam, top_n, 1.0, scorer)
    _identical(got, _whole(dev, probs, sizes, beam, top_n, 1.0, scorer))
    _same(got, ref, beam)
    _distinct(got, ref)


# ---------------------------------------------------------------------------- 4. read-out
@pytest.mark.parametrize("lm", [False, True])
def test_partial_readout_is_the_prefix_decode(dev, lm):
    if lm:
        beam, top_n = 100, 40
        labels, probs, sizes, _ = _lm_case(0, beam, top_n, 0.8, 1.0, 2.0)
        scorer = _scorer(dev, labels)
        parts = [3, 3, 1, 1, 5, 0, 9]
        parts = parts + [probs.shape[1] - sum(parts)]
    else:
        beam, top_n = 10, 40
        probs, sizes, _ = _random_case(beam, top_n, 1.0, 30)
        scorer = None
        parts = [7, 13, 0, 17]
    each_end, each, _ = _streamed(dev, probs, sizes, parts, beam, top_n, 1.0, scorer,
                                  read_each=True)
    for done, got in each:
        if done == 0:
            continue      # (a whole-utterance decode of no frames has no rows to compare)
        pre = [min(s, done) for s in sizes]
        _identical(got, _whole(dev, probs[:, :done], pre, beam, top_n, 1.0, scorer))
    # reading out after every chunk changes nothing that is carried
    only_end, _, _ = _streamed(dev, probs, sizes, parts, beam, top_n, 1.0, scorer)
    _identical(each_end, only_end)
    assert all(torch.equal(x, y) for x, y in zip(each_end[2:], only_end[2:]))


# ---------------------------------------------------------------------------- 5. isolation
def test_streams_are_independent_and_runs_repeat(dev):
    beam, top_n, c = 100, 40, 36
    probs, sizes, ref = _random_case(beam, top_n, 1.0, c)
    parts = [7, 13, 17]
    a, _, state = _streamed(dev, probs, sizes, parts, beam, top_n, 1.0)
    b, _, _ = _streamed(dev, probs, sizes, parts, beam, top_n, 1.0)
    _identical(a, b)                                            # two identical runs
    perm = [3, 0, 4, 2, 1]
    p, _, _ = _streamed(dev, probs[perm], [sizes[i] for i in perm], parts, beam, top_n, 1.0)
    _identical(p, tuple(x[perm] for x in a))                    # a stream's neighbours
    # the same buffers after a reset reproduce the first run
    assert ops.ctc_beam_stream_state(5, 37, beam, dev, out=state) is state
    r, _, _ = _streamed(dev, probs, sizes, parts, beam, top_n, 1.0, state=state)
    _identical(r, a)
    _same(r, ref, beam)


@pytest.mark.parametrize("lm", [False, True])
def test_chunk_without_valid_frames_leaves_a_stream_alone(dev, lm):
    """Stream 0 sits out the second call (0 valid frames, junk in its rows) while stream 1
    advances; afterwards each stream's result is its own whole-utterance decode, and the
    record of stream 0 is the same bytes before and after that call."""
    beam, top_n = 20, 40
    labels = orc.LABELS
    g = np.random.default_rng(5)
    t, c = 30, len(labels)
    probs = _batch([_spelled("THE CAT SAT ON A HAT", g, 2.0, labels)[:t],
                    _spelled("AND THEY SAT ON A CAT", g, 2.0, labels)[:t]], c)
    assert probs.shape[1] == t
    scorer = _scorer(dev, labels) if lm else None
    whole = _whole(dev, probs, [t, t], beam, top_n, 1.0, scorer)
    pd = torch.tensor(probs).to(dev)
    max_frames = t + 5
    state = ops.ctc_beam_stream_state(2, max_frames, beam, dev)
    rec_bytes = 4 * (8 + 14 * ((beam + 3) // 4 * 4))    # one stream's record (csrc/ctc.hip)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)
    _feed(state, pd[:, :10], None, beam, beam, max_frames, 0, False, top_n, 1.0, scorer)
    before = state[:rec_bytes].clone()
    junk = torch.rand(2, 5, c, device=dev)
    junk[1] = pd[1, 10:15]
    out = _feed(state, junk, i32([0, 5]), beam, beam, max_frames, 10, True, top_n, 1.0, scorer)
    assert torch.equal(state[:rec_bytes], before)
    assert out[4].cpu().tolist() == [10, 15]
    # stream 0 can still be read out: its first ten frames
    pre = _whole(dev, probs[:1, :10], [10], beam, top_n, 1.0, scorer)
    _identical(tuple(x[:1].cpu() for x in out[:4]), pre)
    rest = torch.full((2, t - 10, c), 1.0 / c, device=dev)
    rest[0] = pd[0, 10:]
    rest[1, :t - 15] = pd[1, 15:]
    out = _feed(state, rest, i32([t - 10, t - 15]), beam, beam, max_frames, 15, True, top_n, 1.0,
                scorer)
    assert out[4].cpu().tolist() == [t, t]
    _identical(tuple(x.cpu() for x in out[:4]), whole)


def test_no_frame_is_consumed_past_max_frames(dev):
    """The trie is sized for max_frames frames.  The entry refuses a host count past it; a
    caller whose count understates what it fed is held to the bound by the kernel, which
    counts the frames itself: the stream stops at max_frames and says so."""
    from ds2amd import _lib
    beam, top_n = 10, 40
    probs, _, _ = _random_case(beam, top_n, 1.0, 30)
    pd = torch.tensor(probs[:2]).to(dev)
    state = ops.ctc_beam_stream_state(2, 10, beam, dev)
    with pytest.raises(_lib.Ds2Error):
        ops.ctc_beam_stream_feed_raw(state, pd[:, :11], None, beam, beam, 10, 0)
    ops.ctc_beam_stream_feed_raw(state, pd[:, :8], None, beam, beam, 10, 0, readout=False)
    out = ops.ctc_beam_stream_feed_raw(state, pd[:, 8:16], None, beam, beam, 10, 2)   # 8 were fed
    assert out[4].cpu().tolist() == [10, 10]
    _identical(tuple(x.cpu() for x in out[:4]), _whole(dev, probs[:2, :10], [10, 10], beam, top_n, 1.0))
    # a state initialised for another beam width is not advanced
    out = ops.ctc_beam_stream_feed_raw(ops.ctc_beam_stream_state(2, 10, beam, dev), pd[:, :4],
                                       None, beam - 1, 1, 10, 0)
    assert out[4].cpu().tolist() == [-1, -1]
    assert out[2].cpu().tolist() == [[0], [0]]


# ---------------------------------------------------------------------------- 6. decoder
def test_decoder_interface(dev):
    from ds2amd.decoder import BeamCTCDecoder, StreamingBeamCTCDecoder
    beam, top_n = 100, 40
    labels, probs, sizes, ref = _lm_case(0, beam, top_n, 0.8, 1.0, 2.0)
    t = probs.shape[1]
    pd = torch.tensor(probs).to(dev)
    kw = dict(lm_path=ARPA, alpha=0.8, beta=1.0, cutoff_top_n=top_n, beam_width=beam)
    want_s, want_o = BeamCTCDecoder(labels, **kw).decode(pd, torch.tensor(sizes, dtype=torch.int32))
    dec = StreamingBeamCTCDecoder(labels, max_frames=t, top_paths=3, **kw)
    for rnd in range(2):
        done = 0
        for k in [5, 0, 11, t - 16]:
            sz = torch.tensor([min(max(s - done, 0), k) for s in sizes], dtype=torch.int32)
            out = dec.feed(pd[:, done:done + k], sz, partial=(k != 11))
            done += k
            if k == 11:
                assert out is None
                continue
            strings, offsets = out
            assert len(strings) == len(sizes) and all(len(s) == 3 for s in strings)
            assert all(len(o) == 3 for o in offsets)
            for n in range(len(sizes)):
                assert len(offsets[n][0]) == len(strings[n][0])
                assert all(int(v) < done for v in offsets[n][0])
        assert dec.frames_fed == t
        assert [s[:3] for s in want_s] == strings
        for n in range(len(sizes)):
            for p in range(3):
                assert offsets[n][p].tolist() == want_o[n][p].tolist()
        fin_s, fin_o = dec.finish()
        assert fin_s == want_s
        assert all(a.tolist() == b.tolist() for x, y in zip(fin_o, want_o) for a, b in zip(x, y))
        assert dec.text() == [s[0] for s in want_s]
        assert dec.text() == [''.join(labels[i] for i in paths[0][1]) if paths else '' for paths in ref]
        with pytest.raises(ValueError):
            dec.feed(pd[:, :1])                      # past max_frames
        with pytest.raises(ValueError):
            dec.feed(pd[:2, :0])                     # the stream count is fixed
        dec.reset()                                  # second round: the same buffers
        assert dec.frames_fed == 0


def test_streaming_session_into_streaming_beam_decoder(dev):
    """A tiny unidirectional GRU model: StreamingSession.feed -> StreamingBeamCTCDecoder.feed
    over chunks of 16 input frames, then finish; the strings and offsets are
    BeamCTCDecoder.decode's on the concatenation of the same streamed probs."""
    from ds2amd import model as dsm
    from ds2amd.decoder import BeamCTCDecoder, StreamingBeamCTCDecoder
    from ds2amd.streaming import StreamingSession
    torch.manual_seed(11)
    conf = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
    m = dsm.DeepSpeech(rnn_type='gru', labels=orc.LABELS, rnn_hidden_size=32, nb_layers=2,
                       audio_conf=conf, bidirectional=False, context=20).eval().to(dev)
    n, t = 2, 120
    x = torch.randn(n, 1, 161, t, generator=torch.Generator().manual_seed(3)).to(dev)
    session = StreamingSession(m, n_streams=n)
    dec = StreamingBeamCTCDecoder(orc.LABELS, beam_width=20, max_frames=(t - 1) // 2 + 1)
    chunks, texts = [], []
    for a in range(0, t, 16):
        _, probs = session.feed(x[..., a:a + 16].contiguous())
        chunks.append(probs)
        strings, offsets = dec.feed(probs)
        assert len(strings) == n and len(strings[0]) == 1
        texts.append([s[0] for s in strings])
    _, probs = session.finish()
    chunks.append(probs)
    dec.feed(probs, partial=False)
    allp = torch.cat(chunks, 1)
    assert allp.shape[1] == (t - 1) // 2 + 1 == dec.frames_fed
    assert any(c.shape[1] > 0 for c in chunks[:-1])          # the beam was carried across feeds
    strings, offsets = dec.finish()
    want_s, want_o = BeamCTCDecoder(orc.LABELS, beam_width=20).decode(allp)
    assert strings == want_s
    for got, want in zip(offsets, want_o):
        assert len(got) == len(want) == 20
        assert all(a.tolist() == b.tolist() for a, b in zip(got, want))
    assert dec.text() == [s[0] for s in want_s]
