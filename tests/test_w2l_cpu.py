"""CPU: rnn_type='cnn' (Wav2Letter) constructs with the reference's module tree -- state_dict
keys, order, shapes and seeded initial weights of tests/golden/w2l_tiny.npz (made from the
reference's model.py) -- loads the golden state, and round-trips through serialize /
load_model_package.  No kernel runs here."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from ds2amd import model as dsm
from ds2amd.optim import FlatParams, FusedAdam, FusedSGD

import w2l_common as wc


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_state_dict_matches_reference(form):
    m = wc.build_ds2amd(form)
    keys, shapes = wc.golden_keys(form)
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert sd["fc.0.weight"].shape == (30, wc.HIDDEN, 1) and "fc.0.bias" in sd
    assert "rnns.0.bias" not in sd                     # body convolutions have no bias
    # seeded construction draws the reference's initial weights (conv.*: by their sums)
    g = wc.golden()
    for k, v in wc.golden_state(form).items():
        assert torch.equal(sd[k], v), k
    for k in keys:
        if k.startswith("conv."):
            assert sd[k].double().sum().item() == float(g[f"{form}_wsum::{k}"]), k
    assert m.get_seq_lens(torch.IntTensor(g["lengths"])).tolist() == g[f"{form}_out_lengths"].tolist()


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_module_list_is_the_builders(form):
    m = wc.build_ds2amd(form)
    kinds = [type(x).__name__ for x in m.rnns]
    block = ["Conv1d", "BatchNorm1d", "ReLU"] if wc.FORMS[form] else ["Conv1d", "GLUModule", "BatchNorm1d"]
    assert kinds == block * (wc.LAYERS + 3)
    convs = [x for x in m.rnns if isinstance(x, nn.Conv1d)]
    mult = 1 if wc.FORMS[form] else 2
    assert [(c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0])
            for c in convs] == (
        [(161, mult * wc.WIDTH, 13, 2, 6)] + [(wc.WIDTH, mult * wc.WIDTH, 13, 1, 6)] * wc.LAYERS
        + [(wc.WIDTH, mult * wc.HIDDEN, 31, 1, 15), (wc.HIDDEN, mult * wc.HIDDEN, 1, 1, 0)])
    assert all(c.bias is None for c in convs)
    assert isinstance(m.conv, dsm.MaskConv)            # constructed although never called
    assert [id(p) for p in m.unused_parameters()] == [id(p) for p in m.conv.parameters()]
    # nn.Dropout after every block only when dropout > 0 (it shifts the indices)
    torch.manual_seed(0)
    d = dsm.DeepSpeech(rnn_type='cnn', labels=wc.labels(), rnn_hidden_size=8, nb_layers=1,
                       cnn_width=8, dropout=0.25)
    assert [type(x).__name__ for x in d.rnns][:4] == ["Conv1d", "BatchNorm1d", "ReLU", "Dropout"]
    assert "rnns.4.weight" in d.state_dict() and d.rnns[3].p == 0.25


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_load_and_serialize_round_trip(form):
    torch.manual_seed(77)                               # other weights than the golden ones
    m = dsm.DeepSpeech(rnn_type='cnn', labels=wc.labels(), rnn_hidden_size=wc.HIDDEN,
                       nb_layers=wc.LAYERS, audio_conf=wc.AUDIO_CONF,
                       bidirectional=wc.FORMS[form], cnn_width=wc.WIDTH)
    missing, unexpected = m.load_state_dict(wc.golden_state(form), strict=False)
    assert not unexpected and all(k.startswith("conv.") for k in missing)
    pkg = dsm.DeepSpeech.serialize(m, epoch=1)
    assert pkg['rnn_type'] == 'cnn' and pkg['cnn_width'] == wc.WIDTH
    assert pkg['bidirectional'] == wc.FORMS[form] and pkg['dropout'] == 0
    m2 = dsm.DeepSpeech.load_model_package(pkg)
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert m2._rnn_type == 'cnn' and m2._cnn_width == wc.WIDTH


def test_out_of_scope_types_still_raise():
    for t in wc.OUT_OF_SCOPE + ('transformer',):
        with pytest.raises(ValueError, match="cnn"):    # the message names 'cnn' as supported
            dsm.DeepSpeech(rnn_type=t, labels=wc.labels(), rnn_hidden_size=8, nb_layers=1)


def test_bf16_gemm_precision_is_refused():
    with pytest.raises(ValueError, match="cnn"):
        wc.build_ds2amd("relu", rnn_gemm_precision='bf16')
    m = wc.build_ds2amd("relu")
    with pytest.raises(ValueError, match="cnn"):
        m.set_rnn_gemm_precision('bf16')
    assert m.set_rnn_gemm_precision('fp32') is m


def test_forward_needs_the_gpu():
    m = wc.build_ds2amd("relu")
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 1, 161, 20), torch.IntTensor([20]))


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_unused_parameters_stay_outside_the_flat_buffers(opt):
    """conv.* never receives a gradient: it keeps its own storage and .grad None (so no
    update or weight decay reaches it), yet keeps its place in the optimizer's parameter
    order, and the state_dict loads into torch's optimizer over model.parameters()."""
    m = wc.build_ds2amd("glu")
    before = [p.detach().clone() for p in m.conv.parameters()]
    flat = FlatParams(list(m.parameters()), torch.device("cpu"), unused=m.unused_parameters())
    used = {id(p) for p in flat.params}
    assert all(id(p) not in used and p.grad is None for p in m.conv.parameters())
    assert flat.model_params == [p for p in m.parameters()]
    assert flat.numel == sum((p.numel() + 63) // 64 * 64 for p in m.parameters()
                             if id(p) in used)
    assert all(torch.equal(a, b) for a, b in zip(before, m.conv.parameters()))
    if opt == "sgd":
        o = object.__new__(FusedSGD)
        o.flat, o.lr, o.momentum, o.weight_decay, o.steps = flat, 0.1, 0.9, 1e-3, 1
        o.buf = torch.zeros_like(flat.flat)
        ref = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9, nesterov=True,
                              weight_decay=1e-3)
    else:
        o = object.__new__(FusedAdam)
        o.flat, o.lr, o.betas, o.eps, o.weight_decay = flat, 1e-3, (0.9, 0.999), 1e-8, 1e-3
        o.exp_avg = torch.zeros_like(flat.flat)
        o.exp_avg_sq = torch.zeros_like(flat.flat)
        o.step_count = torch.ones(1, dtype=torch.int32)
        ref = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-3)
    sd = o.state_dict()
    n_all = len(list(m.parameters()))
    n_unused = len(m.unused_parameters())
    assert sd['param_groups'][0]['params'] == list(range(n_all))
    assert sorted(sd['state']) == list(range(n_unused, n_all))    # conv.* come first
    ref.load_state_dict(sd)
    o.load_state_dict(sd)
