"""Generate tests/golden/w2l_tiny.npz from the REFERENCE implementation (CPU, build
container only; the tests read the .npz, never the reference).

Run:  python tests/golden/make_w2l_golden.py   (reference checkout: $DS2_REFERENCE, default
/root/reference)

Imports the reference's own model.py, builds DeepSpeech(rnn_type='cnn', rnn_hidden_size=24,
nb_layers=2, cnn_width=16) under a fixed seed in both forms (bidirectional=True: Conv1d ->
BatchNorm1d -> ReLU; False: Conv1d(2 x out) -> GLU -> BatchNorm1d) and runs the forward branch
of model.py:350-352, ``fc(rnns(x.squeeze(1)))``, in float64 (the reference's forward itself
asserts x.is_cuda).  Per form (prefix ``relu_`` / ``glu_``):
  keys, shapes           the ordered state_dict key list and the shapes
  w::<key>               the float32 initial rnns.* / fc.* state
  wsum::<key>            float64 sum of each conv.* tensor (the unused MaskConv stack is not
                         stored: seeded construction reproduces it, the sums prove it)
  train_logits           [3, 30, 19] float64, train mode (batch statistics)
  stat::<key>            running_mean / running_var / num_batches_tracked after that forward
  eval_logits            [3, 30, 19] float64, eval mode on the updated running statistics
and, shared: x [3, 1, 161, 37] float32, lengths (37, 30, 12), out_lengths from get_seq_lens.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DS2_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.modules.setdefault("Levenshtein", types.ModuleType("Levenshtein"))
import model as ref_model      # noqa: E402  (reference model.py)

LABELS = ''.join(json.load(open(os.path.join(REF, 'labels.json'))))
AUDIO_CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
SEED = 1234


def main():
    out = {}
    g = torch.Generator().manual_seed(99)
    lengths = [37, 30, 12]
    x = torch.zeros(3, 1, 161, 37)
    for i, t in enumerate(lengths):
        x[i, 0, :, :t] = torch.randn(161, t, generator=g)
    out["x"] = x.numpy()
    out["lengths"] = np.asarray(lengths, dtype=np.int32)
    out["labels"] = np.asarray(LABELS)
    out["seed"] = np.asarray(SEED)
    for form, bidir in (("relu", True), ("glu", False)):
        torch.manual_seed(SEED)
        m = ref_model.DeepSpeech(rnn_type='cnn', labels=LABELS, rnn_hidden_size=24, nb_layers=2,
                                 audio_conf=AUDIO_CONF, bidirectional=bidir, cnn_width=16)
        sd = m.state_dict()
        out[f"{form}_keys"] = np.asarray(list(sd.keys()))
        out[f"{form}_shapes"] = np.asarray([json.dumps(list(v.shape)) for v in sd.values()])
        for k, v in sd.items():
            if k.startswith("conv."):
                # the unused MaskConv stack (1 MB of random weights): its float64 sum only;
                # the tests rebuild it by seeded construction, which draws the same values
                out[f"{form}_wsum::{k}"] = np.asarray(v.double().sum().item())
            else:
                out[f"{form}_w::{k}"] = v.detach().numpy().copy()
        out[f"{form}_out_lengths"] = m.get_seq_lens(torch.IntTensor(lengths)).numpy().astype(np.int32)
        m = m.double()
        xd = x.double().squeeze(1)
        m.train()
        with torch.no_grad():
            y = m.fc(m.rnns(xd))
        assert tuple(y.shape) == (3, len(LABELS), 19), y.shape
        out[f"{form}_train_logits"] = y.numpy().copy()
        for k, v in m.state_dict().items():
            if k.startswith(("rnns.", "fc.")) and k.rsplit(".", 1)[1] in (
                    "running_mean", "running_var", "num_batches_tracked"):
                out[f"{form}_stat::{k}"] = v.detach().numpy().copy()
        m.eval()
        with torch.no_grad():
            y = m.fc(m.rnns(xd))
        out[f"{form}_eval_logits"] = y.numpy().copy()
    path = os.path.join(HERE, "w2l_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
