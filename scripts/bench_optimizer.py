"""The optimizer tail's four streaming kernels at cfg2's flat size (5 x BiGRU-800: 41,188,768
parameters plus FlatParams' alignment padding, laid out as the Trainer lays them out):
ds2_grad_norm, ds2_clip_sgd_nesterov, ds2_clip_sgd_nesterov_wd, ds2_clip_adam.

Device time per call from HIP events after a warm-up; the kernels take turns over several
rounds (the median round is reported, with the fastest and slowest) so that a drift of the
machine hits all of them alike.  One JSON line per kernel: milliseconds and algorithmic bytes
per second -- 4 B / element for the norm (one read), 20 B for SGD (p, g, buf read; p, buf
written), 28 B for Adam (p, g, m, v read; p, m, v written) -- and, for the two new kernels,
that rate over the decay-free SGD kernel's of the same run.  DS2_LIB_PATH selects the library.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'deepspeech.pytorch_amd'))
from ds2amd import _lib, ops   # noqa: E402
from ds2amd import model as dsm   # noqa: E402
from ds2amd.optim import FlatParams   # noqa: E402

LABELS = "_'ABCDEFGHIJKLMNOPQRSTUVWXYZ2 "
CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')


def cfg2_flat_numel():
    m = dsm.DeepSpeech(rnn_type='gru', labels=LABELS, rnn_hidden_size=800, nb_layers=5,
                       audio_conf=CONF, bidirectional=True)
    pairs = [(x.weight_ih_l0, x.weight_ih_l0_reverse) for x in m.modules()
             if hasattr(x, 'weight_ih_l0_reverse')]
    flat = FlatParams(list(m.parameters()), 'cpu', adjacent=pairs)
    return flat.numel, sum(p.numel() for p in m.parameters())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numel', type=int, default=0, help="flat size (default: cfg2's)")
    ap.add_argument('--reps', type=int, default=50, help="calls per timed window")
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    numel, params = (a.numel, a.numel) if a.numel else cfg2_flat_numel()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer.py times HIP kernels: it needs the GPU")
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    p = (torch.randn(numel, generator=g) * 0.05).to(dev)
    grad = (torch.randn(numel, generator=g) * 1e-2).to(dev)
    buf = torch.zeros(numel, device=dev)
    m = torch.zeros(numel, device=dev)
    v = torch.zeros(numel, device=dev)
    norm = torch.zeros(1, dtype=torch.float32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(16, _lib.size("ds2_optim_workspace_size", numel)), dtype=torch.uint8,
                     device=dev)
    s = ops._stream()
    lr, mom, wd, max_norm = 3e-4, 0.9, 1e-5, 100.0
    kernels = [
        ("ds2_grad_norm", 4, lambda: _lib.call(
            "ds2_grad_norm", grad.data_ptr(), numel, norm.data_ptr(), ws.data_ptr(), ws.numel(),
            s)),
        ("ds2_clip_sgd_nesterov", 20, lambda: _lib.call(
            "ds2_clip_sgd_nesterov", p.data_ptr(), grad.data_ptr(), buf.data_ptr(), numel, lr,
            mom, max_norm, norm.data_ptr(), None, s)),
        ("ds2_clip_sgd_nesterov_wd", 20, lambda: _lib.call(
            "ds2_clip_sgd_nesterov_wd", p.data_ptr(), grad.data_ptr(), buf.data_ptr(), numel, lr,
            mom, wd, max_norm, norm.data_ptr(), None, s)),
        ("ds2_clip_adam", 28, lambda: _lib.call(
            "ds2_clip_adam", p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), numel,
            lr, 0.9, 0.999, 1e-8, wd, max_norm, norm.data_ptr(), step.data_ptr(), None, s)),
    ]
    for _, _, fn in kernels:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in kernels}
    for _ in range(a.rounds):
        for name, _, fn in kernels:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.reps)
    assert torch.isfinite(p).all().item() and int(step.item()) == a.warmup + a.rounds * a.reps
    rate = {}
    for name, per, _ in kernels:
        med = statistics.median(ms[name])
        rate[name] = per * numel / (med * 1e-3)
        row = {"kernel": name, "numel": numel, "parameters": params, "ms": round(med, 5),
               "ms_min": round(min(ms[name]), 5), "ms_max": round(max(ms[name]), 5),
               "bytes_per_element": per, "algorithmic_bytes": per * numel,
               "bytes_per_s": round(rate[name], -6), "reps": a.reps, "rounds": a.rounds}
        if name in ("ds2_clip_sgd_nesterov_wd", "ds2_clip_adam"):
            row["rate_vs_clip_sgd_nesterov"] = round(rate[name] / rate["ds2_clip_sgd_nesterov"], 4)
        print(json.dumps(row))


if __name__ == '__main__':
    main()
