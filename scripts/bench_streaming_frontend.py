#!/usr/bin/env python3
"""The streaming front-end against the only alternative there was: re-running the whole-utterance
STFT on the growing prefix at every chunk.

30 s of 16 kHz audio (n_fft 320, hop 160, 'max_frame').  Sweep: N streams in {1, 8} x chunks of
{16, 32, 64} frames' worth of samples.  Per configuration, in one process and in alternating
rounds after one warm-up pass of each:

  frontend    one StreamingFrontend.feed per chunk (+ finish), the causal offset
  prefix      ops.stft_logmag(normalize=1) on pcm[:, :end] at eight evenly spaced chunk ends
  transcribe  one StreamingTranscriber.feed per chunk: front-end -> StreamingSession (5 x GRU-800
              unidirectional, Lookahead 20) -> StreamingGreedyDecoder

Every call is timed with the host clock around the call and a device synchronise.  Reported per
method: median and maximum latency per call over all rounds and each round's median; for the
front-end also the medians of the first and the last quarter of the feeds (a feed must not
depend on what was fed before) and the device-side events per feed from a separate profiled
pass (torch.profiler, never the timed one; "null" when the profiler reports none).

--tag labels the rows (the frames-per-block build of csrc/stft_stream.hip the library under
DS2_LIB_PATH was compiled with); --append adds to --out instead of replacing it.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_streaming import LABELS, launches_per_call, summarise, timed  # noqa: E402

import torch  # noqa: E402

from ds2amd import model as dsm  # noqa: E402
from ds2amd import ops  # noqa: E402
from ds2amd.data_loader import gaussian_taps  # noqa: E402
from ds2amd.decoder import StreamingGreedyDecoder  # noqa: E402
from ds2amd.streaming import StreamingFrontend, StreamingTranscriber  # noqa: E402

CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
HOP = 160


def frontend_pass(front, pcm, step):
    front.reset()
    lat, frames = [], 0
    for a in range(0, pcm.shape[1], step):
        piece = pcm[:, a:a + step]
        torch.cuda.synchronize()
        ms, out = timed(lambda: front.feed(piece))
        lat.append(ms)
        frames += out.shape[3]
    ms, out = timed(front.finish)
    return lat, ms, frames + out.shape[3]


def prefix_pass(front, pcm, step, taps):
    ends = list(range(step, pcm.shape[1] + 1, step))
    picks = [ends[(i + 1) * len(ends) // 8 - 1] for i in range(8)]
    lat = []
    for end in picks:
        piece = pcm[:, :end].contiguous()
        lens = torch.full((pcm.shape[0],), end, dtype=torch.int32, device=pcm.device)
        frames = ops.stft_frames(end, front.n_fft, front.hop)
        torch.cuda.synchronize()
        ms, _ = timed(lambda: ops.stft_logmag(piece, lens, front.n_fft, front.hop, front._window,
                                              1, taps, frames))
        lat.append(ms)
    return lat, picks


def transcribe_pass(model, pcm, step):
    t = StreamingTranscriber(model, StreamingGreedyDecoder(LABELS), n_streams=pcm.shape[0])
    lat = []
    for a in range(0, pcm.shape[1], step):
        piece = pcm[:, a:a + step]
        torch.cuda.synchronize()
        ms, _ = timed(lambda: t.feed(piece))
        lat.append(ms)
    ms, _ = timed(t.finish)
    return lat, ms


def quarters(rounds):
    q = max(len(rounds[0]) // 4, 1)
    return (round(statistics.median([v for r in rounds for v in r[:q]]), 3),
            round(statistics.median([v for r in rounds for v in r[-q:]]), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "streaming_frontend_bench.jsonl"))
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--chunks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--tag", default="frames_per_block=4")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-transcribe", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_streaming_frontend: no GPU (a CPU run measures nothing about the MI355X)")
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    model = None
    if not args.no_transcribe:
        model = dsm.DeepSpeech(rnn_type='gru', labels=LABELS, rnn_hidden_size=800, nb_layers=5,
                               bidirectional=False, context=20, audio_conf=CONF).to(dev).eval()
    taps = torch.tensor(gaussian_taps(20), dtype=torch.float32, device=dev)
    samples = int(round(args.seconds * CONF['sample_rate']))
    if not args.append:
        open(args.out, "w").close()
    for n in args.streams:
        pcm = torch.randn(n, samples, device=dev, generator=torch.Generator(dev).manual_seed(n))
        pcm = (pcm * 0.1).clamp_(-1, 1)
        front = StreamingFrontend(CONF, n_streams=n, device=dev)
        for chunk in args.chunks:
            step = chunk * HOP
            frontend_pass(front, pcm, step)             # warm-up: every shape of the timed passes
            prefix_pass(front, pcm, step, taps)
            if model is not None:
                transcribe_pass(model, pcm, step)
            f_rounds, p_rounds, t_rounds, finish = [], [], [], []
            for _ in range(args.rounds):                # alternating
                lat, fin, frames = frontend_pass(front, pcm, step)
                assert frames == ops.stft_frames(samples, front.n_fft, front.hop)
                f_rounds.append(lat)
                finish.append(fin)
                lat, picks = prefix_pass(front, pcm, step, taps)
                p_rounds.append(lat)
                if model is not None:
                    t_rounds.append(transcribe_pass(model, pcm, step)[0])
            front.reset()
            front.feed(pcm[:, :8 * step])
            launches = launches_per_call(
                lambda i: front.feed(pcm[:, (8 + i) * step:(9 + i) * step]), 4)
            fe = summarise(f_rounds)
            first, last = quarters(f_rounds)
            fe.update(first_quarter_median_ms=first, last_quarter_median_ms=last,
                      finish_ms=round(statistics.median(finish), 3), launches_per_feed=launches)
            prefix = summarise(p_rounds)
            prefix.update(prefix_ends_samples=picks,
                          per_end_ms=[round(statistics.median(r[i] for r in p_rounds), 3)
                                      for i in range(len(picks))])
            row = dict(tag=args.tag, audio_s=args.seconds, streams=n, chunk_frames=chunk,
                       chunk_ms=chunk * 10.0, rounds=args.rounds, frontend=fe, prefix_rerun=prefix)
            if t_rounds:
                row["transcriber_feed"] = summarise(t_rounds)
                row["transcriber_model"] = "5xGRU-800 unidirectional, Lookahead 20, greedy decoder"
            print(json.dumps(row))
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
