#!/usr/bin/env python
"""The manifest -> batch path against the training step it feeds, at cfg2's shape.

Writes 32 x 10 s of int16 wavs (SURVEY 8(d)'s signal: seeded white Gaussian noise plus three
sinusoids of 100-4000 Hz, peak-normalised) and a manifest that lists them BINS times into a
temporary directory, then in ONE process, in alternating rounds, times

  loader   one epoch of DeviceBatchLoader alone (the device otherwise idle), batches / s,
           with DS2_PCM_DECODE unset and =0, for prefetch 0 and 2;
  step     Trainer.train_batch fed a resident batch, and fed by the loader (prefetch 2).

One JSON line per round and leg goes to --out (default profiles/input_pipeline.jsonl) and
to stdout.  Usage: python scripts/bench_input_pipeline.py [--rounds 5] [--bins 8]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "deepspeech.pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

BATCH, SECONDS, SR, LABEL_LEN = 32, 10, 16000, 150
LABELS = "_'ABCDEFGHIJKLMNOPQRSTUVWXYZ2 "
CONF = dict(sample_rate=SR, window_size=0.02, window_stride=0.01, window='hamming')


def write_corpus(root, bins):
    from scipy.io import wavfile
    rows = []
    for i in range(BATCH):
        rng = np.random.default_rng(1234 + i)
        t = np.arange(SECONDS * SR) / SR
        y = rng.standard_normal(t.shape[0])
        for f in rng.uniform(100, 4000, 3):
            y += np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
        y /= np.abs(y).max()
        wav = os.path.join(root, f"u{i:02d}.wav")
        wavfile.write(wav, SR, np.round(y * 32767).astype(np.int16))
        # LABEL_LEN characters, no two equal neighbours (no '2' codes), words of 5
        chars, prev = [], ''
        while len(chars) < LABEL_LEN:
            space = len(chars) % 6 == 5 and len(chars) < LABEL_LEN - 1
            c = ' ' if space else LABELS[2 + int(rng.integers(26))]
            if c != prev:
                chars.append(c)
                prev = c
        txt = os.path.join(root, f"u{i:02d}.txt")
        with open(txt, "w", encoding="utf8") as f:
            f.write(''.join(chars).lower())
        rows.append((wav, txt))
    man = os.path.join(root, "manifest.csv")
    with open(man, "w", newline="") as f:
        for _ in range(bins):
            f.writelines(f"{w},{t},{SECONDS}\n" for w, t in rows)
    return man


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bins", type=int, default=8, help="batches per epoch")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "input_pipeline.jsonl"))
    args = ap.parse_args()

    from ds2amd import model as dsm
    from ds2amd.data_loader import BucketingSampler, DeviceBatchLoader, SpectrogramDataset
    from ds2amd.trainer import Trainer
    dev = torch.device("cuda", 0)
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    with tempfile.TemporaryDirectory() as root:
        man = write_corpus(root, args.bins)
        ds = SpectrogramDataset(CONF, man, None, LABELS, normalize='max_frame', augment=False,
                                device=dev)
        sampler = BucketingSampler(ds, batch_size=BATCH)

        def epoch(prefetch, consume=None):
            """Seconds per batch over one epoch, device idle at both ends."""
            loader = DeviceBatchLoader(ds, sampler, prefetch=prefetch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for batch in loader:
                if consume is not None:
                    consume(batch)
                n += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n

        def set_decode(on):
            if on:
                os.environ.pop("DS2_PCM_DECODE", None)
            else:
                os.environ["DS2_PCM_DECODE"] = "0"

        torch.manual_seed(123456)
        m = dsm.DeepSpeech(rnn_type='gru', labels=LABELS, rnn_hidden_size=800, nb_layers=5,
                           audio_conf=CONF, bidirectional=True)
        tr = Trainer(m, LABELS, lr=3e-4, momentum=0.9, max_norm=100.0, device=dev, score=True,
                     verbose=False)
        resident = next(iter(DeviceBatchLoader(ds, sampler, prefetch=0)))
        assert tuple(resident[0].shape) == (BATCH, 1, 161, 1001), resident[0].shape
        assert resident[4].tolist() == [LABEL_LEN] * BATCH

        def resident_step(_=None):
            x, tg, names, pct, ts = resident
            tr.train_batch((x, tg, names, pct.clone(), ts))

        def resident_epoch():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.bins):
                resident_step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.bins

        # warm-up: kernels, allocator, pinned staging, page cache
        for on in (True, False):
            set_decode(on)
            epoch(2)
        resident_epoch()

        for r in range(args.rounds):
            for on in (True, False):
                set_decode(on)
                for prefetch in (0, 2):
                    s = epoch(prefetch)
                    emit(round=r, leg="loader", pcm_decode=on, prefetch=prefetch,
                         ms_per_batch=round(s * 1e3, 3), batches_per_s=round(1 / s, 2))
            s = resident_epoch()
            emit(round=r, leg="step_resident", ms_per_step=round(s * 1e3, 3))
            for on in (True, False):
                set_decode(on)
                s = epoch(2, consume=tr.train_batch)
                emit(round=r, leg="step_from_loader", pcm_decode=on, prefetch=2,
                     ms_per_step=round(s * 1e3, 3))
        set_decode(True)
        tr.poll_status(block=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
