#!/usr/bin/env python
"""Time one training step of the Wav2Letter acoustic model (rnn_type='cnn') at the
reference's defaults -- cnn_width 256, hidden_size 800, hidden_layers 6, batch 32 x 10 s
(T = 1001 frames) -- in both forms (ReLU: bidirectional=True; GLU: bidirectional=False).

A step is Trainer.train_batch: forward, CTC, backward, clip, SGD-Nesterov.  The fast path
(fp16x3 implicit-GEMM Conv1d) and DS2_CONV1D=0 (the general fp32 kernels doing the same
model) are timed in the same process, alternating round by round, device-synchronised.
Prints one JSON line per form -- ms_per_step and audio-seconds/s of both paths with their
spread over the rounds, the per-layer FLOP from the shapes -- and appends it to --out.

Achieved TF per kernel comes from a separate profiler run (the profiler slows the step):
    rocprofv3 --kernel-trace --stats -d DIR -o w2l --output-format csv -- python scripts/bench_w2l.py --profile relu
    python scripts/bench_w2l.py --forms relu --kernel-stats DIR/.../w2l_kernel_stats.csv
--profile runs warm-up + --steps fast-path steps of one form and nothing else; --kernel-stats
merges that run's per-kernel times (divided by its step count) into the JSON line.

--dropout P (default 0: everything above, unchanged) times the model built with dropout=P
instead: the HIP dropout fused into the BatchNorm apply pass, DS2_DROPOUT=0 (torch's
nn.Dropout on the same model) and the dropout-free model, alternating round by round in one
process; one JSON line per form, appended to --out (default profiles/w2l_dropout_bench.jsonl).
With --profile the dropout model's steps are followed by as many of the dropout-free model,
so one trace holds the DROP and the plain instantiation of the apply kernel at one shape.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "deepspeech.pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from ds2amd import model as dsm  # noqa: E402
from ds2amd.trainer import Trainer  # noqa: E402

LABELS = "_'ABCDEFGHIJKLMNOPQRSTUVWXYZ "
FORMS = {"relu": True, "glu": False}
# the fp16x3 engine's peak: the dense fp16 matrix-core rate over three products
FP16X3_PEAK_TF = 838.9


def conv_layers(width, size, layers, glu, classes):
    """(name, Cin, Cout, k, stride, pad, needs_dgrad) of every Conv1d, in order."""
    m = 2 if glu else 1
    out = [("prolog", 161, m * width, 13, 2, 6, False)]
    out += [(f"body{i}", width, m * width, 13, 1, 6, True) for i in range(layers)]
    out += [("epilog31", width, m * size, 31, 1, 15, True), ("epilog1", size, m * size, 1, 1, 0, True),
            ("fc", size, classes, 1, 1, 0, True)]
    return out


def flop_table(batch, frames, width, size, layers, glu, classes):
    t, rows = frames, []
    for name, ci, co, k, s, p, dg in conv_layers(width, size, layers, glu, classes):
        to = (t + 2 * p - k) // s + 1
        f = 2.0 * to * batch * co * ci * k
        rows.append({"layer": name, "c_in": ci, "c_out": co, "k": k, "stride": s, "t_out": to,
                     "fwd_gflop": f / 1e9, "step_gflop": f * (3 if dg else 2) / 1e9})
        t = to
    return rows


def make_batch(batch, frames, label_len, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 1, 161, frames, generator=g)
    tl = torch.full((batch,), label_len, dtype=torch.int32)
    tg = torch.randint(1, len(LABELS), (batch * label_len,), generator=g, dtype=torch.int32)
    pct = torch.ones(batch)
    return x, tg, tl, pct


def build(form, args, dropout=0):
    torch.manual_seed(1)
    m = dsm.DeepSpeech(rnn_type='cnn', labels=LABELS, rnn_hidden_size=args.hidden_size,
                       nb_layers=args.hidden_layers, bidirectional=FORMS[form],
                       cnn_width=args.cnn_width, dropout=dropout)
    return Trainer(m, LABELS, lr=1e-4, momentum=0.9, max_norm=100.0, device="cuda:0",
                   verbose=False, decode=False)


def set_path(fast: bool):
    if fast:
        os.environ.pop("DS2_CONV1D", None)
    else:
        os.environ["DS2_CONV1D"] = "0"


def set_dropout_path(hip: bool):
    if hip:
        os.environ.pop("DS2_DROPOUT", None)
    else:
        os.environ["DS2_DROPOUT"] = "0"


def timed_steps(tr, data, n):
    x, tg, tl, pct = data
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.train_batch((x, tg, None, pct.clone(), tl))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def kernel_stats(path, steps):
    """{kernel name: ms per step} from rocprofv3's *_kernel_stats.csv."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            total = row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or "0"
            out[name] = float(total) / 1e6 / steps
    return out


def summarize(ms):
    """median over the rounds, with the spread (each round is the mean of its steps)"""
    return {"ms_per_step": statistics.median(ms), "min": min(ms), "max": max(ms), "rounds": len(ms)}


def bench_dropout(args, data):
    """fused HIP dropout / torch's nn.Dropout (DS2_DROPOUT=0) / the dropout-free model"""
    out_path = args.out or os.path.join(REPO, "profiles", "w2l_dropout_bench.jsonl")
    audio_s = args.batch * (args.frames - 1) / 100.0
    for form in args.forms.split(","):
        tr_p, tr_0 = build(form, args, args.dropout), build(form, args)
        legs = (("fused", tr_p, True), ("torch", tr_p, False), ("none", tr_0, True))
        ms = {name: [] for name, _, _ in legs}
        for _, tr, hip in legs:
            set_dropout_path(hip)
            timed_steps(tr, data, args.warmup)
        for _ in range(args.rounds):
            for name, tr, hip in legs:                                # alternating
                set_dropout_path(hip)
                ms[name].append(timed_steps(tr, data, args.steps))
        set_dropout_path(True)
        tr_p.close()
        tr_0.close()
        res = {k: summarize(v) for k, v in ms.items()}
        for r in res.values():
            r["audio_s_per_s"] = audio_s / (r["ms_per_step"] / 1e3)
        gain = res["torch"]["ms_per_step"] - res["fused"]["ms_per_step"]
        spread = max(r["max"] - r["min"] for r in (res["fused"], res["torch"]))
        line = json.dumps({
            "bench": "w2l_dropout_train_step", "form": form, "dropout": args.dropout,
            "batch": args.batch, "frames": args.frames, "cnn_width": args.cnn_width,
            "hidden_size": args.hidden_size, "hidden_layers": args.hidden_layers,
            "steps_per_round": args.steps, "fused": res["fused"],
            "torch_DS2_DROPOUT_0": res["torch"], "dropout_free": res["none"],
            "torch_over_fused": res["torch"]["ms_per_step"] / res["fused"]["ms_per_step"],
            "fused_over_dropout_free": res["fused"]["ms_per_step"] / res["none"]["ms_per_step"],
            "fused_not_slower": res["fused"]["ms_per_step"] <= res["torch"]["ms_per_step"],
            "gain_ms": gain, "rounds_spread_ms": spread, "gain_inside_spread": gain <= spread})
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--forms", default="relu,glu")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--cnn-width", type=int, default=256)
    ap.add_argument("--hidden-size", type=int, default=800)
    ap.add_argument("--hidden-layers", type=int, default=6)
    ap.add_argument("--label-len", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100,
                    help="fast-path steps per round (a round exceeds a second)")
    ap.add_argument("--general-steps", type=int, default=12,
                    help="DS2_CONV1D=0 steps per round (about ten times slower per step)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="P > 0: time the dropout=P model, fused HIP path against DS2_DROPOUT=0")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--profile", metavar="FORM", default=None,
                    help="profiler mode: warm-up + --steps fast-path steps of FORM only")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of --profile")
    ap.add_argument("--stats-steps", type=int, default=None,
                    help="steps the profiled run took (default: its --warmup + --steps)")
    args = ap.parse_args()

    data = make_batch(args.batch, args.frames, args.label_len)
    if args.profile:
        set_path(True)
        tr = build(args.profile, args, args.dropout)
        ms = timed_steps(tr, data, args.warmup + args.steps)
        rec = {"profile": args.profile, "steps": args.warmup + args.steps,
               "ms_per_step_under_profiler": ms}
        tr.close()
        if args.dropout > 0:      # the dropout-free model next, for the plain apply kernel
            tr = build(args.profile, args)
            rec.update(dropout=args.dropout, dropout_path=os.environ.get("DS2_DROPOUT", "1"),
                       ms_per_step_dropout_free=timed_steps(tr, data, args.warmup + args.steps))
            tr.close()
        print(json.dumps(rec), flush=True)
        return
    if args.dropout > 0:
        bench_dropout(args, data)
        return

    for form in args.forms.split(","):
        tr = build(form, args)
        ms = {"fast": [], "general": []}
        for fast in (True, False):
            set_path(fast)
            timed_steps(tr, data, args.warmup)
        for _ in range(args.rounds):
            for name, fast in (("fast", True), ("general", False)):   # alternating
                set_path(fast)
                ms[name].append(timed_steps(tr, data, args.steps if fast else args.general_steps))
        set_path(True)
        tr.close()
        table = flop_table(args.batch, args.frames, args.cnn_width, args.hidden_size,
                           args.hidden_layers, not FORMS[form], len(LABELS))
        audio_s = args.batch * (args.frames - 1) / 100.0
        fast, gen = summarize(ms["fast"]), summarize(ms["general"])
        out = {"bench": "w2l_train_step", "form": form, "batch": args.batch, "frames": args.frames,
               "cnn_width": args.cnn_width, "hidden_size": args.hidden_size,
               "hidden_layers": args.hidden_layers,
               "steps_per_round": {"fast": args.steps, "general": args.general_steps},
               "fast": dict(fast, audio_s_per_s=audio_s / (fast["ms_per_step"] / 1e3)),
               "general_DS2_CONV1D_0": dict(gen, audio_s_per_s=audio_s / (gen["ms_per_step"] / 1e3)),
               "speedup": gen["ms_per_step"] / fast["ms_per_step"],
               "fast_not_slower": fast["ms_per_step"] <= gen["ms_per_step"],
               "fwd_tflop": sum(r["fwd_gflop"] for r in table) / 1e3,
               "step_tflop": sum(r["step_gflop"] for r in table) / 1e3,
               "step_tf_per_s": sum(r["step_gflop"] for r in table) / fast["ms_per_step"],
               "layers": table}
        if args.kernel_stats:
            steps = args.stats_steps or (args.warmup + args.steps)
            ks = kernel_stats(args.kernel_stats, steps)
            conv = {k: v for k, v in ks.items() if "c1_" in k}
            # the fast kernels' work: every layer with k > 1 (the 1x1 layers run on the GEMM)
            igemm_gflop = sum(r["step_gflop"] - r["fwd_gflop"] for r in table if r["k"] > 1)
            wgrad_gflop = sum(r["fwd_gflop"] for r in table if r["k"] > 1)
            t_ig = sum(v for k, v in conv.items() if "c1_igemm" in k)
            t_wg = sum(v for k, v in conv.items() if "c1_wgrad_kernel" in k)
            out["kernels_ms_per_step"] = dict(sorted(ks.items(), key=lambda kv: -kv[1])[:12])
            if t_ig > 0:
                out["c1_igemm"] = {"ms": t_ig, "tf_per_s": igemm_gflop / t_ig,
                                   "of_fp16x3_peak": igemm_gflop / t_ig / FP16X3_PEAK_TF}
            if t_wg > 0:
                out["c1_wgrad"] = {"ms": t_wg, "tf_per_s": wgrad_gflop / t_wg,
                                   "of_fp16x3_peak": wgrad_gflop / t_wg / FP16X3_PEAK_TF}
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
