#!/usr/bin/env python3
"""Beam search over a stream against the only alternative there was: BeamCTCDecoder.decode on
the growing prefix at every chunk.

Input: a 30 s utterance per stream as the acoustic model would emit it (1500 output frames of
29-label probabilities, peaked on a spelled sentence over the committed tiny_lm.arpa vocabulary,
seeded).  Sweep: chunks of k in {8, 16, 32} output frames x N streams in {1, 8} x beam in
{10, 100} x {no LM, LM}.  Per configuration, in one process and in alternating rounds after one
warm-up pass of each:

  streaming   one StreamingBeamCTCDecoder.feed per chunk (top_paths = 1, read out every call),
              and the same feeds with partial=False (the search alone, no read-out)
  prefix      BeamCTCDecoder.decode(probs[:, :end]) at chunk ends; its cost depends only on
              `end`, so --prefix-samples evenly spaced chunk ends are timed, not every one

Every call is timed with the host clock around the call and a device synchronise (the time a
caller waits for the chunk's text).  Reported per method: median and maximum latency per call
over all rounds and each round's median (the spread); for streaming also the medians of the
first and the last quarter of the utterance (a feed should not cost more late than early) and
microseconds per frame and stream.

Writes one JSON line per configuration to --out (default profiles/streaming_beam_bench.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "deepspeech.pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ds2amd.decoder import BeamCTCDecoder, StreamingBeamCTCDecoder  # noqa: E402

LABELS = "_'ABCDEFGHIJKLMNOPQRSTUVWXYZ "
ARPA = os.path.join(REPO, "tests", "golden", "tiny_lm.arpa")
SENTENCE = "THE CAT SAT ON A HAT AND THEY SAT ON A CAT I DON'T NO THEN CATS IN THEN TOO "
OUT_FRAME_S = 0.02


def spelled(frames, seed, noise=2.0, peak=5.0, blank_bias=1.0):
    """[frames, C] probabilities: every character of the sentence (repeated) as one peaked
    frame followed by a blank one, Gaussian logit noise on top"""
    g = np.random.default_rng(seed)
    idx, prev, i = [], None, 0
    while len(idx) < frames:
        ch = SENTENCE[i % len(SENTENCE)]
        i += 1
        if ch == prev:
            idx.append(0)
        idx += [LABELS.index(ch), 0]
        prev = ch
    idx = idx[:frames]
    logits = g.standard_normal((frames, len(LABELS))).astype(np.float32) * noise
    logits[:, 0] += blank_bias
    logits[np.arange(frames), idx] += peak
    p = np.exp(logits - logits.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def streaming_pass(dec, probs, k, partial):
    dec.reset()
    lat = []
    for a in range(0, probs.shape[1], k):
        piece = probs[:, a:a + k]
        torch.cuda.synchronize()
        ms, _ = timed(lambda: dec.feed(piece, partial=partial))
        lat.append(ms)
    return lat


def prefix_pass(dec, probs, ends):
    lat = []
    for end in ends:
        piece = probs[:, :end]
        torch.cuda.synchronize()
        ms, _ = timed(lambda: dec.decode(piece))
        lat.append(ms)
    return lat


def summarise(rounds):
    flat = [v for r in rounds for v in r]
    return dict(median_ms=round(statistics.median(flat), 3), max_ms=round(max(flat), 3),
                round_medians_ms=[round(statistics.median(r), 3) for r in rounds],
                calls_per_pass=len(rounds[0]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "streaming_beam_bench.jsonl"))
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--beams", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--prefix-samples", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_streaming_beam: no GPU (a CPU run measures nothing about the MI355X)")
    dev = torch.device("cuda:0")
    t = int(round(args.seconds / OUT_FRAME_S))
    open(args.out, "w").close()
    for lm in (False, True):
        for beam in args.beams:
            kw = dict(beam_width=beam, cutoff_top_n=40)
            if lm:
                kw.update(lm_path=ARPA, alpha=0.8, beta=1.0)
            whole = BeamCTCDecoder(LABELS, **kw)
            for n in args.streams:
                probs = torch.from_numpy(np.stack([spelled(t, 100 + i) for i in range(n)])).to(dev)
                dec = StreamingBeamCTCDecoder(LABELS, max_frames=t, top_paths=1, **kw)
                for k in args.chunks:
                    chunk_ends = list(range(k, t + 1, k)) + ([t] if t % k else [])
                    step = max(1, len(chunk_ends) // args.prefix_samples)
                    ends = chunk_ends[step - 1::step]
                    streaming_pass(dec, probs, k, True)       # warm-up of every timed shape
                    streaming_pass(dec, probs, k, False)
                    prefix_pass(whole, probs, ends)
                    s_rounds, d_rounds, p_rounds = [], [], []
                    for _ in range(args.rounds):              # alternating
                        s_rounds.append(streaming_pass(dec, probs, k, True))
                        text = dec.text()
                        d_rounds.append(streaming_pass(dec, probs, k, False))
                        assert dec.text() == text
                        p_rounds.append(prefix_pass(whole, probs, ends))
                    assert text == [s[0] for s in whole.decode(probs)[0]]   # the same answer
                    stream = summarise(s_rounds)
                    q = max(1, len(s_rounds[0]) // 4)
                    stream.update(
                        first_quarter_median_ms=round(statistics.median(
                            [v for r in s_rounds for v in r[:q]]), 3),
                        last_quarter_median_ms=round(statistics.median(
                            [v for r in s_rounds for v in r[-q:]]), 3),
                        chunk_ms=k * OUT_FRAME_S * 1e3)
                    search = summarise(d_rounds)
                    search.update(
                        first_quarter_median_ms=round(statistics.median(
                            [v for r in d_rounds for v in r[:q]]), 3),
                        last_quarter_median_ms=round(statistics.median(
                            [v for r in d_rounds for v in r[-q:]]), 3),
                        us_per_frame_and_stream=round(search["median_ms"] * 1e3 / (k * n), 2))
                    prefix = summarise(p_rounds)
                    prefix.update(prefix_frames=ends, per_end_median_ms=[
                        round(statistics.median(r[i] for r in p_rounds), 3)
                        for i in range(len(ends))])
                    row = dict(audio_s=args.seconds, output_frames=t, lm=lm, beam_width=beam,
                               streams=n, chunk_frames=k, rounds=args.rounds, feed=stream,
                               feed_no_readout=search, prefix_rerun=prefix)
                    print(json.dumps(row), flush=True)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
