#!/usr/bin/env python3
"""Streaming inference against the only alternative there was: re-running the whole-utterance
forward on the growing prefix at every chunk.

Model: 5 x GRU-800 unidirectional with Lookahead 20 (seeded weights, eval), 30 s of audio (3000
spectrogram frames at the 10 ms stride).  Sweep: N streams in {1, 8} x chunks of {16, 32, 64}
input frames.  Per configuration, in one process and in alternating rounds after one warm-up
pass of each:

  streaming   one StreamingSession.feed per chunk (+ finish)
  prefix      model(x[..., :end], lengths=[end] * N) at every chunk end

Every call is timed with the host clock around the call and a device synchronise (the time a
caller waits for the chunk's result).  Reported per method: median and maximum latency per
call over all rounds, each round's median (the spread), audio seconds per second (N x 30 s
over the pass's summed latencies) and, for streaming, whether the median call fits inside the
chunk's own duration.  Launches per call are counted in a separate profiled pass
(torch.profiler, never the timed one): the device-side events of a steady-state call, i.e.
kernels plus the memsets and copies between them; "null" when the profiler reports none.

Writes one JSON line per configuration to --out (default profiles/streaming_bench.jsonl).
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

import torch  # noqa: E402

from ds2amd import model as dsm  # noqa: E402
from ds2amd.streaming import StreamingSession  # noqa: E402

LABELS = "_'ABCDEFGHIJKLMNOPQRSTUVWXYZ "
FRAME_S = 0.01


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def streaming_pass(model, x, chunk):
    s = StreamingSession(model, n_streams=x.shape[0])
    lat, frames = [], 0
    for a in range(0, x.shape[3], chunk):
        piece = x[..., a:a + chunk].contiguous()
        torch.cuda.synchronize()
        ms, (lg, _) = timed(lambda: s.feed(piece))
        lat.append(ms)
        frames += lg.shape[1]
    ms, (lg, _) = timed(s.finish)
    return lat, ms, frames + lg.shape[1]


def prefix_pass(model, x, chunk):
    lat = []
    n, t = x.shape[0], x.shape[3]
    with torch.no_grad():
        for a in range(0, t, chunk):
            end = min(t, a + chunk)
            piece = x[..., :end].contiguous()
            lengths = torch.full((n,), end, dtype=torch.int32)
            torch.cuda.synchronize()
            ms, _ = timed(lambda: model(piece, lengths))
            lat.append(ms)
    return lat


def launches_per_call(fn, calls):
    """device-side events (kernels, memsets, copies) per call over `calls` calls of fn(i), from
    a profiled pass; None when the profiler reports none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for i in range(calls):
                fn(i)
            torch.cuda.synchronize()
        kernels = sum(1 for e in prof.events()
                      if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return round(kernels / calls, 1) if kernels else None
    except Exception as exc:    # the measurement is optional, the reason is reported
        print(f"[bench_streaming] launch count not measured: {exc!r}", file=sys.stderr)
        return None


def summarise(rounds):
    flat = [v for r in rounds for v in r]
    return dict(median_ms=round(statistics.median(flat), 3), max_ms=round(max(flat), 3),
                round_medians_ms=[round(statistics.median(r), 3) for r in rounds],
                calls_per_pass=len(rounds[0]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "streaming_bench.jsonl"))
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--chunks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--hidden", type=int, default=800)
    ap.add_argument("--layers", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_streaming: no GPU (a CPU run measures nothing about the MI355X)")
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    model = dsm.DeepSpeech(rnn_type='gru', labels=LABELS, rnn_hidden_size=args.hidden,
                           nb_layers=args.layers, bidirectional=False, context=20,
                           audio_conf=dict(sample_rate=16000, window_size=0.02,
                                           window_stride=0.01)).to(dev).eval()
    t = int(round(args.seconds / FRAME_S))
    t_out = (t - 1) // 2 + 1
    open(args.out, "w").close()
    for n in args.streams:
        x = torch.randn(n, 1, 161, t, device=dev, generator=torch.Generator(dev).manual_seed(n))
        for chunk in args.chunks:
            streaming_pass(model, x, chunk)         # warm-up: every shape of the timed passes
            prefix_pass(model, x, chunk)
            s_rounds, p_rounds, finish = [], [], []
            for _ in range(args.rounds):            # alternating
                lat, fin, frames = streaming_pass(model, x, chunk)
                assert frames == t_out, (frames, t_out)
                s_rounds.append(lat)
                finish.append(fin)
                p_rounds.append(prefix_pass(model, x, chunk))
            sess = StreamingSession(model, n_streams=n)
            for a in range(0, 8 * chunk, chunk):    # past the latency: steady-state feeds
                sess.feed(x[..., a:a + chunk].contiguous())
            s_launch = launches_per_call(
                lambda i: sess.feed(x[..., (8 + i) * chunk:(9 + i) * chunk].contiguous()), 4)
            half = torch.full((n,), t // 2, dtype=torch.int32)
            with torch.no_grad():
                p_launch = launches_per_call(
                    lambda i: model(x[..., :t // 2].contiguous(), half), 2)
            audio = n * t * FRAME_S
            stream = summarise(s_rounds)
            stream.update(finish_ms=round(statistics.median(finish), 3), launches_per_call=s_launch,
                          audio_s_per_s=round(audio / (min(sum(r) for r in s_rounds)
                                                       + min(finish)) * 1e3, 1),
                          chunk_ms=chunk * FRAME_S * 1e3)
            stream["median_within_chunk"] = stream["median_ms"] <= stream["chunk_ms"]
            stream["max_within_chunk"] = stream["max_ms"] <= stream["chunk_ms"]
            prefix = summarise(p_rounds)
            prefix.update(launches_per_call=p_launch,
                          audio_s_per_s=round(audio / min(sum(r) for r in p_rounds) * 1e3, 1))
            row = dict(model=f"{args.layers}xGRU-{args.hidden} unidirectional, Lookahead 20",
                       audio_s=args.seconds, streams=n, chunk_frames=chunk, rounds=args.rounds,
                       streaming=stream, prefix_rerun=prefix)
            print(json.dumps(row))
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
