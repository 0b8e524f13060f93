"""The prefix beam search's third kernel instance: beams of 33..128 over 33..64 labels (the
reference's Cyrillic label set of 36 at its default beam_width of 100), against the CPU
oracles oracle/ctc_beam.py and oracle/ctc_beam_lm.py: ids, char frames and lengths of every
returned beam bit-exact, scores to 1e-5 relative -- what tests/test_gpu_ops.py asks of the
two older instances, with its generators restated here."""
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
CHUNK = 64   # frames the wide instance stages in LDS at a time (BEAM_WIDE_TCH, csrc/ctc.hip)


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


# ---------------------------------------------------------------------------- comparisons
def _run(dev, probs, sizes, beam, top_n, cutoff, scorer=None):
    pd = torch.tensor(probs).to(dev)   # a copy: the shared reference inputs stay as they are
    sd = torch.tensor(sizes, dtype=torch.int32).to(dev)
    if scorer is None:
        out = ops.ctc_beam_decode_raw(pd, sd, beam, beam, cutoff_top_n=top_n, cutoff_prob=cutoff)
    else:
        out = ops.ctc_beam_decode_lm_raw(pd, sd, beam, beam, scorer, cutoff_top_n=top_n,
                                         cutoff_prob=cutoff)
    return tuple(x.cpu() for x in out)


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


def _valid(got):
    """The defined part of the outputs: rows (n, p) up to lens[n, p]."""
    ids, offs, lens, sc = got
    m = torch.arange(ids.shape[2])[None, None, :] < lens[:, :, None]
    return ids * m, offs * m, lens, sc


# ---------------------------------------------------------------------------- no LM
@pytest.mark.parametrize("beam,top_n,cutoff,c", [
    (100, 40, 1.0, 36),    # the Russian case: the reference's default beam over its labels
    (128, 40, 1.0, 64),    # both maxima
    (128, 64, 1.0, 64),    # no pruning: every one of 8192 candidates live
    (33, 64, 1.0, 33),     # both minima of the instance
    (65, 40, 1.0, 40),     # beam entries cross one per-lane boundary
    (100, 10, 0.99, 48),   # both cutoffs
])
def test_wide_beam_vs_oracle(dev, beam, top_n, cutoff, c):
    probs, sizes, ref = _random_case(beam, top_n, cutoff, c)
    _same(_run(dev, probs, sizes, beam, top_n, cutoff), ref, beam)


@pytest.mark.parametrize("beam,top_n,cutoff,c", [(32, 40, 1.0, 64), (128, 40, 1.0, 32)])
def test_older_instances_still_routed(dev, beam, top_n, cutoff, c):
    """The shapes at the edge of the new dispatch rule that the two older instances keep."""
    probs, sizes, ref = _random_case(beam, top_n, cutoff, c)
    _same(_run(dev, probs, sizes, beam, top_n, cutoff), ref, beam)


def test_wide_beam_is_deterministic(dev):
    beam, top_n, cutoff, c = 128, 64, 1.0, 64
    probs, sizes, ref = _random_case(beam, top_n, cutoff, c)
    a = _valid(_run(dev, probs, sizes, beam, top_n, cutoff))
    b = _valid(_run(dev, probs, sizes, beam, top_n, cutoff))
    _same(a, ref, beam)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))   # scores: same bits


# ---------------------------------------------------------------------------- LM
@pytest.mark.parametrize("extra", [6, 3, 34])
@pytest.mark.parametrize("beam,top_n,cutoff,alpha,beta,noise",
                         [(100, 40, 1.0, 0.8, 1.0, 2.0), (33, 8, 1.0, 1.2, 0.5, 3.0),
                          (128, 64, 1.0, 0.8, 1.0, 3.0)])
def test_wide_beam_lm_vs_oracle(dev, extra, beam, top_n, cutoff, alpha, beta, noise):
    """Noisy spelled sentences (test_ctc_beam_lm_vs_oracle's) plus sizes 0 and 1, over 36, 33
    and 64 labels; through BeamCTCDecoder(lm_path=...) the best strings are the oracle's."""
    from oracle import ctc_beam_lm as obl
    from ds2amd.lm import ArpaScorer
    from ds2amd.decoder import BeamCTCDecoder
    labels = WIDE(extra)
    g = np.random.default_rng(beam * 7 + top_n)
    texts = ["THE CAT SAT ", "I DON'T NO ", "AND THEY SAT ON A HAT", "CATS IN THEN"]
    ps = [_spelled(s, g, noise, labels) for s in texts]
    probs = _batch(ps, len(labels), extra=2)
    sizes = [p.shape[0] for p in ps] + [0, 1]
    scorer = ArpaScorer(ARPA, labels, alpha, beta, device=dev)
    got = _run(dev, probs, sizes, beam, top_n, cutoff, scorer)
    ref = obl.beam_decode_lm(probs, sizes, beam, obl.ArpaLM(ARPA), labels, alpha, beta,
                             cutoff_top_n=top_n, cutoff_prob=cutoff)
    _same(got, ref, beam)
    dec = BeamCTCDecoder(labels, lm_path=ARPA, alpha=alpha, beta=beta, cutoff_top_n=top_n,
                         cutoff_prob=cutoff, beam_width=beam)
    strings, _ = dec.decode(torch.from_numpy(probs).to(dev), torch.tensor(sizes, dtype=torch.int32))
    for n, paths in enumerate(ref):
        assert len(strings[n]) == beam
        assert strings[n][0] == (''.join(labels[i] for i in paths[0][1]) if paths else '')


# ---------------------------------------------------------------------------- revival
@pytest.mark.parametrize("extra,beam,top_n,plain_revives", [(34, 128, 40, True), (34, 128, 64, True),
                                                           (3, 100, 40, False)])
def test_wide_beam_trie_revival_vs_oracle(dev, extra, beam, top_n, plain_revives):
    """test_ctc_beam_trie_revival_vs_oracle's sentences at noise 3.0: the oracle revives
    pruned prefixes (over 64 labels in both searches, over 33 with the LM only), both device
    searches equal it bit-exactly and every returned beam holds distinct strings."""
    from oracle import ctc_beam, ctc_beam_lm as obl
    from ds2amd.lm import ArpaScorer
    labels = WIDE(extra)
    g = np.random.default_rng(11)
    ps = [_spelled(s, g, 3.0, labels) for s in ["THE CAT SAT ON A HAT", "I DON'T NO THEN ",
                                                "AND THEY SAT ON A CAT", "CATS IN THEN TOO"]]
    probs = _batch(ps, len(labels))
    sizes = [p.shape[0] for p in ps]
    ctc_beam.STATS["revived"] = 0
    ref = ctc_beam.beam_decode(probs, sizes, beam, cutoff_top_n=top_n, cutoff_prob=1.0)
    if plain_revives:
        assert ctc_beam.STATS["revived"] > 0
    got = _run(dev, probs, sizes, beam, top_n, 1.0)
    _same(got, ref, beam)
    _distinct(got, ref)
    ctc_beam.STATS["revived"] = 0
    ref = obl.beam_decode_lm(probs, sizes, beam, obl.ArpaLM(ARPA), labels, 0.8, 1.0,
                             cutoff_top_n=top_n, cutoff_prob=1.0)
    assert ctc_beam.STATS["revived"] > 0
    got = _run(dev, probs, sizes, beam, top_n, 1.0, ArpaScorer(ARPA, labels, 0.8, 1.0, device=dev))
    _same(got, ref, beam)
    _distinct(got, ref)


# ---------------------------------------------------------------------------- staging
@pytest.mark.parametrize("lm", [False, True])
def test_wide_beam_staging_boundary(dev, lm):
    """Utterances of 2 CHUNK + 3 frames (two full chunks and a tail of three) and of exactly
    CHUNK frames (no second chunk), c = 40, beam 64."""
    from oracle import ctc_beam, ctc_beam_lm as obl
    from ds2amd.lm import ArpaScorer
    labels = WIDE(10)
    beam = 64
    g = np.random.default_rng(64)
    text = "THE CAT SAT ON A HAT AND THEY SAT ON A CAT I DON'T NO THEN CATS IN THEN TOO "
    long_p = _spelled(text, g, 2.0, labels)[:2 * CHUNK + 3]
    one_p = _spelled(text[20:], g, 2.0, labels)[:CHUNK]
    assert long_p.shape[0] == 2 * CHUNK + 3 and one_p.shape[0] == CHUNK
    probs = _batch([long_p, one_p], len(labels))
    sizes = [2 * CHUNK + 3, CHUNK]
    if lm:
        ref = obl.beam_decode_lm(probs, sizes, beam, obl.ArpaLM(ARPA), labels, 0.8, 1.0)
        got = _run(dev, probs, sizes, beam, 40, 1.0, ArpaScorer(ARPA, labels, 0.8, 1.0, device=dev))
    else:
        ref = ctc_beam.beam_decode(probs, sizes, beam, cutoff_top_n=40, cutoff_prob=1.0)
        got = _run(dev, probs, sizes, beam, 40, 1.0)
    assert len(ref[0]) == beam and len(ref[0][0][1]) > 20    # a full beam of long prefixes
    _same(got, ref, beam)
