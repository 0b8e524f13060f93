"""GPU: the XCD-local GRU recurrences (csrc/gru_xl.hip) run with fewer tiles per wave than the
instantiation holds -- the waves leave their MFMA chains early, and the fragments of the
producers they do not have are zeros -- and the timeout path of such a launch.
"""
import pytest
import torch

from ds2amd import _lib, ops

pytestmark = pytest.mark.gpu


def _close(got, ref, rel, name):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


def _lens(t, n):
    return torch.tensor(sorted([t - (i % 6) * 5 for i in range(n)], reverse=True),
                        dtype=torch.int32)


def _gru_run(dev, n, t, inp, h, nd, seed, env, monkeypatch):
    """One GRU layer forward + backward per environment in `env`, seeded weights, ragged
    lengths (tests/test_gpu_gru_handoff.py's helper); [y, dx, dW...] per run."""
    g = torch.Generator().manual_seed(seed)
    a = h ** -0.5
    weights = [torch.rand(s, generator=g) * 2 * a - a for s in
               [(3 * h, inp), (3 * h, h), (3 * h,), (3 * h,)] * nd]
    lens = _lens(t, n)
    x = torch.randn(t, n, inp, generator=g)
    dy = torch.randn(t, n, h, generator=g)
    outs = []
    for e in env:
        for k, v in e.items():
            monkeypatch.setenv(k, v)
        ws = [w.to(dev).requires_grad_(True) for w in weights]
        xd = x.to(dev).requires_grad_(True)
        y = ops.GRULayerFn.apply(xd, lens.to(dev), True, h, *ws)
        y.backward(dy.to(dev))
        torch.cuda.synchronize()
        ops.check_rnn_status(dev)
        outs.append([y.detach().cpu(), xd.grad.cpu()] + [w.grad.cpu() for w in ws])
    return outs


# H / 32 producers over the 4 waves: 9 = (3, 2, 2, 2) and 13 = (4, 3, 3, 3) on the instances
# built for 3 + 1, 17 = (5, 4, 4, 4) -- every wave below its build count -- and 21 = (6, 5, 5,
# 5) on those built for 6 + 1
@pytest.mark.parametrize("t,n,h,bidir", [(27, 9, 288, True), (29, 8, 416, False),
                                         (31, 12, 544, True), (33, 5, 672, False)])
def test_gru_xl_partial_instances(dev, t, n, h, bidir, monkeypatch):
    """Outputs and every gradient finite; a second run bit-identical; every group forced GLOBAL
    (DS2_GRU_XL=2) bit-identical; within 2e-5 of the fp32-MFMA kernels (DS2_GRU_X6=0); and the
    shape is one the XCD-local launch takes: the backward's grid covers its nd x ceil(n / 8)
    groups of h / 32 workgroups, and the 16-unit kernels (DS2_GRU_XL=0), whose sums run in
    another order, do not give the same bits -- so the case did not pass on a fallback rung."""
    nd = 2 if bidir else 1
    monkeypatch.setenv("DS2_GRU_XL", "1")
    monkeypatch.setenv("DS2_GRU_X6", "1")
    xl_grid = nd * ((n + 7) // 8) * (h // 32)
    grid = ops.persistent_bwd_grid("gru", n, h, nd)
    monkeypatch.setenv("DS2_GRU_XL", "0")
    grid_off = ops.persistent_bwd_grid("gru", n, h, nd)
    assert grid == max(xl_grid, grid_off), (grid, xl_grid, grid_off)
    env = [{"DS2_GRU_XL": "1", "DS2_GRU_X6": "1"}, {"DS2_GRU_XL": "1"}, {"DS2_GRU_XL": "2"},
           {"DS2_GRU_XL": "1", "DS2_GRU_X6": "0"}, {"DS2_GRU_XL": "0", "DS2_GRU_X6": "1"}]
    loc, again, glob, f32, u16 = _gru_run(dev, n, t, 40, h, nd, h + 7 * n, env, monkeypatch)
    for i, (a, b, c, d) in enumerate(zip(loc, again, glob, f32)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(a, b), f"output {i}: second run differs"
        assert torch.equal(a, c), f"output {i}: GLOBAL differs from LOCAL"
        _close(a, d, 2e-5, f"output {i}: XCD-local vs fp32 MFMA")
    assert any(not torch.equal(a, e) for a, e in zip(loc, u16)), \
        "bit-identical to the 16-unit kernels: the XCD-local launch declined the shape"


def test_gru_xl_timeout_partial_instance(dev, monkeypatch):
    """Spin bound 0 at h = 544 (waves with 5 and 4 of 7 tiles): every wait reports a timeout at
    once, the MFMAs that still run read whatever the tiles hold, the kernels fill their
    remaining outputs with NaN and return, and check_rnn_status raises; with the bound
    restored the same layer runs clean."""
    t, n, h = 31, 12, 544
    g = torch.Generator().manual_seed(5)
    a = h ** -0.5
    ws = [(torch.rand(s, generator=g) * 2 * a - a).to(dev) for s in
          [(3 * h, 40), (3 * h, h), (3 * h,), (3 * h,)] * 2]
    x = torch.randn(t, n, 40, generator=g).to(dev)
    lens = _lens(t, n).to(dev)
    ops.rnn_status_word(dev).zero_()
    monkeypatch.setenv("DS2_RNN_SPIN_LIMIT", "0")
    monkeypatch.setenv("DS2_RNN_TUNE", "1,0")
    xd = x.clone().requires_grad_(True)
    y = ops.GRULayerFn.apply(xd, lens, True, h, *ws)     # forward and backward both time out
    y.backward(torch.ones_like(y))
    with pytest.raises(_lib.Ds2Error, match="hand-off"):
        ops.check_rnn_status(dev)
    assert torch.isnan(y).any()
    monkeypatch.delenv("DS2_RNN_SPIN_LIMIT")
    monkeypatch.delenv("DS2_RNN_TUNE")
    with torch.no_grad():
        y = ops.GRULayerFn.apply(x, lens, True, h, *ws)
    torch.cuda.synchronize()
    ops.check_rnn_status(dev)
    assert torch.isfinite(y).all()
