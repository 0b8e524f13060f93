"""CTC forced alignment at the bench shape (T' = 501, 32 utterances, 29 classes, label lengths
drawn around 150) next to the CTC loss on the same inputs.  One process alternates three calls,
ops.ctc_align_raw, ops.ctc_loss_raw(want_grad=True) and ops.ctc_loss_raw(want_grad=False):
every round times `--reps` launches of each between CUDA events, and the per-launch times of
the rounds (median, min, max) are printed and, with --out, written to a file.  The alignment is
also checked against the loss on the way: its score can never exceed -cost."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'deepspeech.pytorch_amd'))
from ds2amd import ops   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(3)
    t, n, c = 501, 32, 29
    lens = torch.randint(130, 171, (n,), generator=g, dtype=torch.int32)
    max_l = int(lens.max())
    acts = (torch.randn(t, n, c, generator=g) * 2).to(dev)
    labels = torch.randint(1, c, (int(lens.sum()),), generator=g, dtype=torch.int32).to(dev)
    act_lens = torch.full((n,), t, dtype=torch.int32, device=dev)
    label_lens = lens.to(dev)
    calls = {
        'ctc_align_raw': lambda: ops.ctc_align_raw(acts, labels, act_lens, label_lens, max_l),
        'ctc_loss_raw(want_grad=True)': lambda: ops.ctc_loss_raw(
            acts, labels, act_lens, label_lens, max_l, want_grad=True),
        'ctc_loss_raw(want_grad=False)': lambda: ops.ctc_loss_raw(
            acts, labels, act_lens, label_lens, max_l, want_grad=False),
    }
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    scores = calls['ctc_align_raw']()[2]
    costs = calls['ctc_loss_raw(want_grad=False)']()[0]
    assert torch.isfinite(scores).all() and (scores <= -costs + 1e-3 * costs.abs()).all()
    times = {name: [] for name in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for name, fn in calls.items():
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
    lines = [f"# scripts/bench_ctc_align.py on {arch}: T'={t}, N={n}, "
             f"C={c}, label lengths {int(lens.min())}..{max_l}; us per launch over "
             f"{args.rounds} rounds of {args.reps} launches, the three calls alternating"]
    for name, v in times.items():
        lines.append(f"{name:32s} median {statistics.median(v):8.1f}  min {min(v):8.1f}  "
                     f"max {max(v):8.1f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + "\n")


if __name__ == '__main__':
    main()
