"""GPU: the HIP dropout of the Wav2Letter blocks (ds2_dropout_apply, ds2_bn_dropout_apply_amax,
ds2_bn_relu_dropout_bwd) against the host Philox reference of dropout_common, bit for bit where
the arithmetic is the existing kernels' times one float multiply; the model with dropout = 0.2
against a float64 restatement with the same masks, within w2l_common.bound of the float32 CPU
run's own distance from float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ds2amd import _lib, ops
from ds2amd import model as dsm

import dropout_common as dc
import w2l_common as wc

pytestmark = pytest.mark.gpu

SEED, OFFSET = dc.SEED, dc.OFFSET
UNSUPPORTED = 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _expect(y0, keep, p):
    """where(keep, y0 * float32(1 / (1 - p)), 0) in float32, as the kernels form it"""
    return np.where(keep, y0.astype(np.float32) * dc.scale32(p), np.float32(0.0))


def _same_bits(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32),
                          np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


# ------------------------------------------------------------------ 1. the mask, bit-exact
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("shape", [(1, 4), (7, 12), (3, 5), (69, 260)])
def test_mask_bit_exact(dev, shape, p):
    x = torch.ones(shape, device=dev)
    y = ops.dropout_apply(x, p, SEED, OFFSET)
    keep = dc.keep_mask(shape, p, SEED, OFFSET)
    assert _same_bits(y, _expect(np.ones(shape, np.float32), keep, p))
    assert torch.equal(y, ops.dropout_apply(x, p, SEED, OFFSET))          # same (seed, offset)
    if shape == (69, 260):
        assert not torch.equal(y, ops.dropout_apply(x, p, SEED, OFFSET + 4))   # offsets 8, 12
        assert not np.array_equal(keep, dc.keep_mask(shape, p, SEED, OFFSET + 4))


def test_mask_unaligned_operand_and_in_place(dev):
    """a 4-byte aligned view takes the element-by-element path: the same mask"""
    base = torch.randn(7 * 12 + 1, device=dev)
    x = base[1:].view(7, 12)
    assert x.data_ptr() % 16 == 4
    keep = dc.keep_mask((7, 12), 0.2, SEED, OFFSET)
    want = _expect(x.cpu().numpy(), keep, 0.2)
    assert _same_bits(ops.dropout_apply(x, 0.2, SEED, OFFSET), want)
    assert _same_bits(ops.dropout_apply(x, 0.2, SEED, OFFSET, out=x), want)


@pytest.mark.parametrize("shape", [(3, 5), (69, 260)])
def test_p_zero_is_identity_and_p_one_is_zero(dev, shape):
    x = torch.randn(shape, device=dev)
    assert _same_bits(ops.dropout_apply(x, 0.0, SEED, OFFSET), x.cpu().numpy())
    y = ops.dropout_apply(x, 1.0, SEED, OFFSET)
    assert _same_bits(y, np.zeros(shape, np.float32))


# ------------------------------------------------------------------ 2. the fused forward
def _bn_operands(rows, c, dev, seed=3):
    g = torch.Generator().manual_seed(seed + rows * 4099 + c)
    x = torch.randn(rows, c, generator=g) * 2 + 0.5
    mean = torch.randn(c, generator=g) * 0.3
    invstd = torch.rand(c, generator=g) + 0.5
    gamma = torch.randn(c, generator=g)
    beta = torch.randn(c, generator=g) * 0.2
    return [t.to(dev) for t in (x, mean, invstd, gamma, beta)]


def _unfused(x, mean, invstd, gamma, beta, relu):
    """the existing apply-with-maxima entry (needs the fused shape conditions)"""
    r, c = x.shape
    y = torch.empty_like(x)
    rm = torch.empty(r, dtype=torch.int32, device=x.device)
    cm = torch.empty(c, dtype=torch.int32, device=x.device)
    _lib.call("ds2_bn_relu_apply_amax" if relu else "ds2_bn_apply_amax", x.data_ptr(), r, c,
              mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
              rm.data_ptr(), cm.data_ptr(), _stream())
    return y


def _fused(x, mean, invstd, gamma, beta, relu, p, seed, offset):
    r, c = x.shape
    y = torch.full_like(x, float("nan"))
    rm = torch.full((r,), -1, dtype=torch.int32, device=x.device)
    cm = torch.full((c,), -1, dtype=torch.int32, device=x.device)
    st = _lib.load().ds2_bn_dropout_apply_amax(
        x.data_ptr(), r, c, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
        relu, p, seed, offset, y.data_ptr(), rm.data_ptr(), cm.data_ptr(), _stream())
    return st, y, rm, cm


def _check_fused(x, bn, relu, p, offset):
    st, y, rm, cm = _fused(x, *bn, relu, p, SEED, offset)
    assert st == 0
    keep = dc.keep_mask(tuple(x.shape), p, SEED, offset)
    want = _expect(_unfused(x, *bn, relu).cpu().numpy(), keep, p)
    assert _same_bits(y, want)
    a = np.abs(want)
    assert np.array_equal(rm.cpu().numpy().view(np.float32), a.max(axis=1))
    assert np.array_equal(cm.cpu().numpy().view(np.float32), a.max(axis=0))
    return keep, rm


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", [(1, 4), (5, 16), (9, 260), (70, 516), (3, 2048)])
def test_fused_forward_bit_exact(dev, shape, relu):
    x, *bn = _bn_operands(*shape, dev)
    _check_fused(x, bn, relu, 0.2, OFFSET)


@pytest.mark.parametrize("relu", [0, 1])
def test_fused_forward_whole_rows_dropped(dev, relu):
    """p = 0.9 on (6, 4): at the offset chosen here the reference mask drops a whole row (its
    row maximum is 0) and keeps something elsewhere"""
    shape = (6, 4)
    offset = next(o for o in range(0, 4000, 4)
                  if (~dc.keep_mask(shape, 0.9, SEED, o)).all(axis=1).any()
                  and dc.keep_mask(shape, 0.9, SEED, o).any())
    x, *bn = _bn_operands(*shape, dev)
    keep, rm = _check_fused(x, bn, relu, 0.9, offset)
    dead = ~keep.any(axis=1)
    assert dead.any() and (rm.cpu().numpy()[dead] == 0).all()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", [(4, 6), (4, 2052)])
def test_fused_unsupported_shapes_fall_back_in_ops(dev, shape, relu):
    x, *bn = _bn_operands(*shape, dev)
    st, _, _, _ = _fused(x, *bn, relu, 0.2, SEED, OFFSET)
    assert st == UNSUPPORTED
    del ops._OPERAND_AMAX[:]
    y = ops.bn_dropout_apply_amax(x, *bn, bool(relu), (0.2, SEED, OFFSET))
    assert not ops._OPERAND_AMAX                      # no maxima kept on the fallback
    y0 = torch.empty_like(x)
    r, c = shape
    if relu:
        _lib.call("ds2_bn_relu_apply", x.data_ptr(), r, c, *[t.data_ptr() for t in bn],
                  y0.data_ptr(), _stream())
    else:
        _lib.call("ds2_bn_apply", x.data_ptr(), r, c, 1, *[t.data_ptr() for t in bn],
                  y0.data_ptr(), _stream())
    keep = dc.keep_mask(shape, 0.2, SEED, OFFSET)
    assert _same_bits(y, _expect(y0.cpu().numpy(), keep, 0.2))


def test_fused_p_zero_and_p_one(dev):
    x, *bn = _bn_operands(9, 260, dev)
    st, y, rm, cm = _fused(x, *bn, 1, 0.0, SEED, OFFSET)
    assert st == 0 and _same_bits(y, _unfused(x, *bn, 1).cpu().numpy())
    st, y, rm, cm = _fused(x, *bn, 1, 1.0, SEED, OFFSET)
    assert st == 0 and not y.any() and not rm.any() and not cm.any()


# ------------------------------------------------------------------ 3. the fused backward
def _relu_bwd(name, dy, y, x, bn, extra=()):
    r, c = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(c, device=x.device)
    db = torch.empty(c, device=x.device)
    ws = torch.empty(_lib.size("ds2_bn_relu_bwd_workspace_size", r, c) + 16, dtype=torch.uint8,
                     device=x.device)
    _lib.call(name, dy.data_ptr(), y.data_ptr(), x.data_ptr(), r, c, *[t.data_ptr() for t in bn],
              *extra, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
              _stream())
    return dx, dg, db


@pytest.mark.parametrize("shape", [(5, 16), (9, 260), (70, 516)])
def test_fused_backward_bit_exact(dev, shape):
    p = 0.2
    x, _, _, gamma, beta = _bn_operands(*shape, dev)
    r, c = shape
    mean, invstd = ops.bn_stats(x, r, c, 1, 1e-5, 0.1, None, None, True)
    bn = [mean, invstd, gamma, beta]
    st, y, _, _ = _fused(x, *bn, 1, p, SEED, OFFSET)
    assert st == 0
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(17)).to(dev)
    got = _relu_bwd("ds2_bn_relu_dropout_bwd", dy, y, x, bn, extra=(p,))
    scaled = torch.from_numpy(dy.cpu().numpy() * dc.scale32(p)).to(dev)      # float32 multiply
    want = _relu_bwd("ds2_bn_relu_bwd", scaled, y, x, bn)
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, want):
        assert _same_bits(a, b.cpu().numpy()), name
    if shape != (70, 516):
        return
    # float64 autograd of mask * scale * relu(bn(x)) over the batch statistics
    keep = torch.from_numpy(dc.keep_mask(shape, p, SEED, OFFSET))
    ref = {}
    for dt in (torch.float64, torch.float32):
        xr = x.cpu().to(dt).requires_grad_(True)
        g = gamma.cpu().to(dt).requires_grad_(True)
        b = beta.cpu().to(dt).requires_grad_(True)
        out = F.relu(F.batch_norm(xr, None, None, g, b, True, 0.1, 1e-5)) \
            * (keep.to(dt) * float(dc.scale32(p)))
        out.backward(dy.cpu().to(dt))
        ref[dt] = (xr.grad, g.grad, b.grad)
    fails = []
    for name, a, r64, r32 in zip(("dx", "dgamma", "dbeta"), got, ref[torch.float64],
                                 ref[torch.float32]):
        d32, ours = wc.rel(r32, r64), wc.rel(a, r64)
        print(f"{name}: d32 {d32:.3e} ours {ours:.3e} bound {wc.bound(d32):.3e}")
        if not ours <= wc.bound(d32):
            fails.append(name)
    assert not fails, fails


# ------------------------------------------------------------------ 4. the model
P = 0.2
N_DROP = 4          # prolog, one body block, the two epilog blocks


def _inputs():
    g = wc.golden()
    return torch.from_numpy(g["x"]), torch.from_numpy(g["lengths"])


def _model(form, dev):
    torch.manual_seed(5)
    return dsm.DeepSpeech(rnn_type='cnn', labels=wc.labels(), rnn_hidden_size=wc.HIDDEN,
                          nb_layers=1, audio_conf=wc.AUDIO_CONF, bidirectional=wc.FORMS[form],
                          cnn_width=wc.WIDTH, dropout=P).to(dev).train()


def _net_items(items):
    return [(k, v) for k, v in items if k.startswith(("rnns.", "fc."))]


def _restatement(m, form, dtype):
    """the torch restatement holding m's weights (the Dropout modules shift m's indices, so the
    tensors are matched in order)"""
    ref = dc.torch_w2l(form, torch.float32, layers=1)
    src, dst = _net_items(m.state_dict().items()), list(ref.state_dict().items())
    assert [tuple(v.shape) for _, v in src] == [tuple(v.shape) for _, v in dst]
    ref.load_state_dict({kd: vs.detach().cpu() for (kd, _), (_, vs) in zip(dst, src)})
    return ref.to(dtype).train()


def _gen(dev):
    return torch.cuda.default_generators[dev.index or 0]


def _step(m, x, lengths, R):
    for p in m.parameters():
        p.grad = None
    logits, _, _ = m(x, lengths)
    (logits * R).sum().backward()
    return logits.detach().clone(), [p.grad.clone() for _, p in _net_items(m.named_parameters())]


def _weights(dev):
    return torch.randn(3, 19, 30, generator=torch.Generator().manual_seed(41),
                       dtype=torch.float64)


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_model_parity_with_explicit_masks(dev, form):
    x, lengths = _inputs()
    R = _weights(dev)
    m = _model(form, dev)
    torch.manual_seed(77)
    seed, off0 = _gen(dev).initial_seed(), _gen(dev).get_offset()
    logits, grads = _step(m, x.to(dev), lengths, R.float().to(dev))
    assert _gen(dev).get_offset() == off0 + 4 * N_DROP
    t, n = logits.shape[1], logits.shape[0]
    chans = [wc.WIDTH, wc.WIDTH, wc.HIDDEN, wc.HIDDEN]
    masks = [dc.keep_mask((t * n, c), P, seed, off0 + 4 * b) for b, c in enumerate(chans)]
    out = {}
    for dt in (torch.float64, torch.float32):
        ref = _restatement(m, form, dt)
        lg = dc.w2l_masked_forward(ref, x, masks, P)
        (lg * R.to(dt)).sum().backward()
        out[dt] = (lg.detach(), [p.grad for p in ref.parameters()])
    names = [k for k, _ in _net_items(m.named_parameters())]
    fails = []
    for name, got, r64, r32 in zip(["logits"] + names, [logits] + grads,
                                   [out[torch.float64][0]] + out[torch.float64][1],
                                   [out[torch.float32][0]] + out[torch.float32][1]):
        d32, ours = wc.rel(r32, r64), wc.rel(got, r64)
        line = f"{form} {name}: d32 {d32:.3e} ours {ours:.3e} bound {wc.bound(d32):.3e}"
        print(line)
        if not ours <= wc.bound(d32):
            fails.append(line)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_model_reproducible_under_seed_and_rng_state(dev, form):
    x, lengths = _inputs()
    xd, R = x.to(dev), _weights(dev).float().to(dev)
    m = _model(form, dev)
    torch.manual_seed(123)
    a = _step(m, xd, lengths, R)
    torch.manual_seed(123)
    b = _step(m, xd, lengths, R)
    assert torch.equal(a[0], b[0]) and all(torch.equal(u, v) for u, v in zip(a[1], b[1]))
    torch.manual_seed(124)
    c = _step(m, xd, lengths, R)
    assert not torch.equal(a[0], c[0])
    assert any(not torch.equal(u, v) for u, v in zip(a[1], c[1]))
    state = torch.cuda.get_rng_state(dev)
    d = _step(m, xd, lengths, R)
    e = _step(m, xd, lengths, R)                      # the stream moved on: another mask
    assert not torch.equal(d[0], e[0])
    torch.cuda.set_rng_state(state, dev)
    f = _step(m, xd, lengths, R)
    assert torch.equal(d[0], f[0]) and all(torch.equal(u, v) for u, v in zip(d[1], f[1]))


def test_eval_mode_consumes_no_offset(dev):
    x, lengths = _inputs()
    m = _model("relu", dev).eval()
    off = _gen(dev).get_offset()
    with torch.no_grad():
        a, _, _ = m(x.to(dev), lengths)
        b, _, _ = m(x.to(dev), lengths)
    assert _gen(dev).get_offset() == off and torch.equal(a, b)


def _record_conv1d(monkeypatch, seen):
    orig = ops.conv1d_fwd

    def wrapped(x, weight, bias, stride, padding, x_row_amax=None):
        y = orig(x, weight, bias, stride, padding, x_row_amax=x_row_amax)
        seen.append((x_row_amax, y, orig(x, weight, bias, stride, padding, x_row_amax=None)))
        return y

    monkeypatch.setattr(ops, "conv1d_fwd", wrapped)


@pytest.mark.parametrize("form", list(wc.FORMS))
def test_scales_handed_to_the_next_conv1d(dev, form, monkeypatch):
    """every Conv1d after the prolog receives the row maxima the fused BatchNorm + dropout
    pass kept, and computes with them what it computes from its own"""
    x, lengths = _inputs()
    m = _model(form, dev)
    seen = []
    _record_conv1d(monkeypatch, seen)
    m(x.to(dev), lengths)
    assert len(seen) == 5 and seen[0][0] is None
    for amax, y, y_own in seen[1:]:
        assert amax is not None
        assert torch.equal(y, y_own)


def test_switch_keeps_the_torch_path(dev, monkeypatch):
    x, lengths = _inputs()
    monkeypatch.setenv("DS2_DROPOUT", "0")
    m = _model("relu", dev)
    seen = []
    _record_conv1d(monkeypatch, seen)
    logits, _, _ = m(x.to(dev), lengths)
    logits.sum().backward()
    assert torch.isfinite(logits).all() and m.rnns[0].weight.grad is not None
    assert torch.isfinite(m.rnns[0].weight.grad).all()
    assert all(amax is None for amax, _, _ in seen)       # torch's dropout made a new tensor
