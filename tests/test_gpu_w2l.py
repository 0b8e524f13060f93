"""GPU: the Wav2Letter acoustic model (rnn_type='cnn') end to end on the golden tiny model
(tests/golden/w2l_tiny.npz, made from the reference's model.py), both forms: forward against
the golden float64 values; backward, two training steps, decode and checkpoints against the
float64 restatement in w2l_common.

Tolerance (per tensor, max abs error over max |ref|): the same restatement run in float32 on
the CPU stands d32 from float64; the HIP result must be within max(2 d32, 1e-5) -- another
summation order is one more draw of that rounding error.  Every comparison appends its d32 and
ours to profiles/w2l_parity.txt when DS2_W2L_PARITY_OUT names a file.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ds2amd import model as dsm
from ds2amd.decoder import GreedyDecoder
from ds2amd.trainer import Trainer

import w2l_common as wc

pytestmark = pytest.mark.gpu


def _check(name, got, ref64, ref32, failures):
    d32 = wc.rel(ref32, ref64)
    ours = wc.rel(got, ref64)
    line = f"{name}: d32 {d32:.3e} ours {ours:.3e} bound {wc.bound(d32):.3e}"
    print(line)
    out = os.environ.get("DS2_W2L_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    if not ours <= wc.bound(d32):
        failures.append(line)


def _inputs():
    g = wc.golden()
    return torch.from_numpy(g["x"]), torch.from_numpy(g["lengths"])


def _hip_model(form, dev):
    m = wc.build_ds2amd(form)
    m.load_state_dict(wc.golden_state(form), strict=False)
    return m.to(dev)


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_forward_matches_golden(dev, form):
    g = wc.golden()
    x, lengths = _inputs()
    m = _hip_model(form, dev).train()
    r32 = wc.torch_w2l(form, torch.float32).train()
    fails = []
    logits, probs, out_lens = m(x.to(dev), lengths)
    with torch.no_grad():
        l32 = r32(x)
    ref = torch.from_numpy(g[f"{form}_train_logits"]).transpose(1, 2)      # [N,T',C]
    assert tuple(logits.shape) == (3, 19, 30) and out_lens.dtype == torch.int32
    assert out_lens.is_cuda and out_lens.cpu().tolist() == g[f"{form}_out_lengths"].tolist()
    _check(f"{form} train logits", logits, ref, l32, fails)
    _check(f"{form} train probs", probs, F.softmax(ref, -1), F.softmax(l32, -1), fails)
    sd, sd32 = m.state_dict(), r32.state_dict()
    for k in g.files:
        if k.startswith(f"{form}_stat::"):
            key = k.split("::", 1)[1]
            if key.endswith("num_batches_tracked"):
                assert int(sd[key]) == int(g[k]) == 1
            else:
                _check(f"{form} {key}", sd[key], torch.from_numpy(g[k]), sd32[key], fails)
    m.eval()
    r32.eval()
    with torch.no_grad():
        logits, probs, _ = m(x.to(dev), lengths)
        l32 = r32(x)
    ref = torch.from_numpy(g[f"{form}_eval_logits"]).transpose(1, 2)
    _check(f"{form} eval logits", logits, ref, l32, fails)
    _check(f"{form} eval probs", probs, F.softmax(ref, -1), F.softmax(l32, -1), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_backward_matches_float64(dev, form):
    x, lengths = _inputs()
    R = torch.randn(3, 19, 30, generator=torch.Generator().manual_seed(41), dtype=torch.float64)
    grads = {}
    for dt in (torch.float64, torch.float32):
        r = wc.torch_w2l(form, dt).train()
        (r(x.to(dt)) * R.to(dt)).sum().backward()
        grads[dt] = {k: p.grad for k, p in r.named_parameters()}
    m = _hip_model(form, dev).train()
    logits, _, _ = m(x.to(dev), lengths)
    (logits * R.float().to(dev)).sum().backward()
    fails = []
    named = dict(m.named_parameters())
    for k, g64 in grads[torch.float64].items():
        assert named[k].grad is not None, k
        _check(f"{form} grad {k}", named[k].grad, g64, grads[torch.float32][k], fails)
    assert all(p.grad is None for p in m.conv.parameters())     # never read, no gradient
    assert not fails, "\n".join(fails)


def _batch():
    g = wc.golden()
    x, lengths = _inputs()
    pct = lengths.float() / float(x.size(3))
    sizes = pct.clone().mul_(int(x.size(3))).int()              # train.py:557, as train_batch
    tl = torch.IntTensor([5, 4, 2])
    tg = torch.randint(1, 30, (int(tl.sum()),), generator=torch.Generator().manual_seed(8),
                       dtype=torch.int32)
    return x, pct, sizes, tg, tl


def _ref_train(form, dt, opt, steps, out_lens):
    x, pct, sizes, tg, tl = _batch()
    r = wc.torch_w2l(form, dt).train()
    if opt == "sgd":
        o = torch.optim.SGD(r.parameters(), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-3)
    else:
        o = torch.optim.Adam(r.parameters(), lr=1e-3, weight_decay=1e-3)
    losses = []
    for _ in range(steps):
        logits = r(x.to(dt)).transpose(0, 1)                    # T x N x C
        loss = F.ctc_loss(F.log_softmax(logits, -1), tg.long(), out_lens.long(), tl.long(),
                          blank=0, reduction='sum') / x.size(0)
        o.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(r.parameters(), 100)
        o.step()
        losses.append(loss.detach())
    return r, o, losses


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("form", list(wc.FORMS))
def test_two_training_steps(dev, form, opt):
    """Two Trainer.train_batch steps (CTC, clip 100, SGD-Nesterov / Adam, weight_decay 1e-3)
    against the float64 restatement with torch's optimizer; conv.* bit-unchanged; the
    optimizer state_dict loads into torch's optimizer over model.parameters()."""
    x, pct, sizes, tg, tl = _batch()
    m = _hip_model(form, dev)
    out_lens = m.get_seq_lens(sizes)
    conv0 = [p.detach().cpu().clone() for p in m.conv.parameters()]
    kw = dict(lr=1e-2, momentum=0.9) if opt == "sgd" else dict(lr=1e-3)
    tr = Trainer(m, wc.labels(), max_norm=100.0, device=dev, verbose=False, optimizer=opt,
                 weight_decay=1e-3, **kw)
    losses = [tr.train_batch((x, tg, None, pct.clone(), tl), return_item=True) for _ in range(2)]
    tr.close()
    r64, _, l64 = _ref_train(form, torch.float64, opt, 2, out_lens)
    r32, _, l32 = _ref_train(form, torch.float32, opt, 2, out_lens)
    fails = []
    for i in range(2):
        _check(f"{form} {opt} loss step {i}", torch.tensor(losses[i]), l64[i], l32[i], fails)
    sd, sd32 = m.state_dict(), r32.state_dict()
    for k, v in r64.state_dict().items():
        if not k.endswith("num_batches_tracked"):
            _check(f"{form} {opt} after 2 steps {k}", sd[k], v, sd32[k], fails)
    for p, p0 in zip(m.conv.parameters(), conv0):
        assert p.grad is None and torch.equal(p.detach().cpu(), p0)
    # reference-ordered torch optimizer (model.parameters(): conv.*, rnns.*, fc.*)
    host = copy.deepcopy(m).cpu()
    ref_opt = (torch.optim.SGD(host.parameters(), lr=1e-2, momentum=0.9, nesterov=True,
                               weight_decay=1e-3) if opt == "sgd"
               else torch.optim.Adam(host.parameters(), lr=1e-3, weight_decay=1e-3))
    sd_o = tr.optimizer.state_dict()
    ref_opt.load_state_dict(sd_o)
    n_conv = len(list(m.conv.parameters()))
    assert sorted(sd_o['state']) == list(range(n_conv, len(list(m.parameters()))))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_decode_and_checkpoint(dev, form):
    """GreedyDecoder on the eval probs = the decode of the golden eval logits' softmax; a
    package in the reference's serialize format loads and reproduces the eval logits."""
    g = wc.golden()
    x, lengths = _inputs()
    # the state after the golden train forward: the initial weights + the golden statistics
    state = wc.golden_state(form)
    for k in g.files:
        if k.startswith(f"{form}_stat::"):
            key = k.split("::", 1)[1]
            state[key] = torch.from_numpy(g[k]).to(state[key].dtype)
    donor = wc.build_ds2amd(form)
    full = donor.state_dict()
    full.update(state)
    package = {'version': '0.0.1', 'hidden_size': wc.HIDDEN, 'hidden_layers': wc.LAYERS,
               'rnn_type': 'cnn', 'audio_conf': wc.AUDIO_CONF, 'labels': wc.labels(),
               'state_dict': full, 'bnm': 0.1, 'bidirectional': wc.FORMS[form], 'dropout': 0,
               'cnn_width': wc.WIDTH}
    m = dsm.DeepSpeech.load_model_package(package).to(dev).eval()
    with torch.no_grad():
        logits, probs, out_lens = m(x.to(dev), lengths)
    ref = torch.from_numpy(g[f"{form}_eval_logits"]).transpose(1, 2)
    r32 = wc.torch_w2l(form, torch.float32)
    r32.load_state_dict({k: v for k, v in state.items()}, strict=True)
    with torch.no_grad():
        l32 = r32.eval()(x)
    fails = []
    _check(f"{form} package eval logits", logits, ref, l32, fails)
    assert not fails, "\n".join(fails)
    dec = GreedyDecoder(wc.labels())
    strings, _ = dec.decode(probs, out_lens)
    ref_strings, _ = dec.decode(F.softmax(ref, -1).float().to(dev), out_lens)
    assert strings == ref_strings and len(strings) == 3


def test_dropout_model_runs(dev):
    """dropout > 0: nn.Dropout modules in the list (torch's dropout, the one non-HIP op);
    eval mode is deterministic and equals the dropout-free network on the same weights."""
    x, lengths = _inputs()
    torch.manual_seed(5)
    d = dsm.DeepSpeech(rnn_type='cnn', labels=wc.labels(), rnn_hidden_size=wc.HIDDEN,
                       nb_layers=1, cnn_width=wc.WIDTH, dropout=0.2).to(dev)
    d.train()
    logits, _, _ = d(x.to(dev), lengths)
    logits.sum().backward()
    assert torch.isfinite(logits).all() and d.rnns[0].weight.grad is not None
    d.eval()
    with torch.no_grad():
        a, _, _ = d(x.to(dev), lengths)
        b, _, _ = d(x.to(dev), lengths)
    assert torch.equal(a, b)
