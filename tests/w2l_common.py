"""Shared by the Wav2Letter tests (not a test module): the golden fixture and a restatement
of the reference's rnn_type='cnn' network from plain torch modules in the builder's order
(model.py:506-562, forward model.py:350-352), run on the CPU in float64 (the reference) or
float32 (one more draw of the float32 rounding error: the tolerance's yardstick)."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w2l_tiny.npz")
AUDIO_CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
FORMS = {"relu": True, "glu": False}        # form -> bidirectional (= not_glu)
HIDDEN, LAYERS, WIDTH = 24, 2, 16
OUT_OF_SCOPE = ('cnn_residual', 'cnn_jasper', 'large_cnn', 'glu_small', 'glu_large')

_G = {}


def golden():
    if "g" not in _G:
        _G["g"] = np.load(GOLDEN)
    return _G["g"]


def labels():
    return str(golden()["labels"])


def golden_keys(form):
    g = golden()
    return [str(k) for k in g[f"{form}_keys"]], [tuple(__import__("json").loads(str(s)))
                                                 for s in g[f"{form}_shapes"]]


def golden_state(form):
    """rnns.* / fc.* tensors of the golden initial state (conv.* is not stored)."""
    g = golden()
    pre = f"{form}_w::"
    return {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def build_ds2amd(form, **kw):
    """The ds2amd model under the golden seed (draws the golden weights), on the CPU."""
    from ds2amd import model as dsm
    torch.manual_seed(int(golden()["seed"]))
    return dsm.DeepSpeech(rnn_type='cnn', labels=labels(), rnn_hidden_size=HIDDEN,
                          nb_layers=LAYERS, audio_conf=AUDIO_CONF, bidirectional=FORMS[form],
                          cnn_width=WIDTH, **kw)


class _GLU(nn.Module):
    def forward(self, x):
        return F.glu(x, dim=1)


class TorchW2L(nn.Module):
    """rnns / fc of the reference's 'cnn' model from torch modules, same order and keys."""

    def __init__(self, not_glu, size=HIDDEN, width=WIDTH, layers=LAYERS, classes=30, bnm=0.1):
        super().__init__()

        def block(i, o, k, p=0, s=1):
            oo = o if not_glu else 2 * o
            res = [nn.Conv1d(i, oo, k, padding=p, stride=s, bias=False)]
            if not_glu:
                res += [nn.BatchNorm1d(oo, momentum=bnm), nn.ReLU()]
            else:
                res += [_GLU(), nn.BatchNorm1d(o, momentum=bnm)]
            return res

        mods = block(161, width, 13, 6, 2)
        for _ in range(layers):
            mods += block(width, width, 13, 6)
        mods += block(width, size, 31, 15)
        mods += block(size, size, 1)
        self.rnns = nn.Sequential(*mods)
        self.fc = nn.Sequential(nn.Conv1d(size, classes, 1))

    def forward(self, x):
        """x [N,1,161,T] -> logits [N,T',C] (model.py:350-353, 375)."""
        return self.fc(self.rnns(x.squeeze(1))).transpose(1, 2)


def torch_w2l(form, dtype):
    m = TorchW2L(FORMS[form], classes=len(labels()))
    m.load_state_dict(golden_state(form), strict=True)
    return m.to(dtype)


def rel(got, ref):
    """max |got - ref| / max |ref|"""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def bound(d32):
    """HIP float32 within max(2 d32, 1e-5): a different summation order is one more draw of
    the rounding error the float32 CPU restatement shows against float64."""
    return max(2.0 * d32, 1e-5)
