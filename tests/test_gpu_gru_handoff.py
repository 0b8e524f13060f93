"""GPU: the XCD-local GRU recurrences (csrc/gru_xl.hip) at the producers-per-wave splits of
their hand-off loops, and the dgx row maxima the backward keeps for the dX GEMM
(ds2_gru_row_amax) against ds2_amax's.
"""
import pytest
import torch

from ds2amd import ops

pytestmark = pytest.mark.gpu


def _close(got, ref, rel=1e-5, name=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


def _lens(t, n):
    return torch.tensor(sorted([t - (i % 6) * 5 for i in range(n)], reverse=True),
                        dtype=torch.int32)


def _gru_run(dev, n, t, inp, h, nd, seed, env, monkeypatch, amp=None):
    """tests/test_gpu_ops.py's helper: one GRU layer forward + backward per environment in
    `env`, seeded weights, ragged lengths; [y, dx, dW...] per run."""
    g = torch.Generator().manual_seed(seed)
    a = amp if amp is not None else (0.2 if h <= 64 else h ** -0.5)
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


# H / 32 producers over the 4 waves of a workgroup: (1, 0, 0, 0) -- empty waves --, 2 = (1, 1,
# 0, 0), 5 = (2, 1, 1, 1), 8 = 2 each, 25 = (7, 6, 6, 6) with the 7th fragment set from LDS,
# 28 = 7 each; whole and partial 8-sample tiles, one and two directions
@pytest.mark.parametrize("t,n,h,bidir", [(23, 8, 32, False), (29, 20, 64, True),
                                         (31, 9, 160, False), (37, 13, 256, True),
                                         (41, 32, 800, True), (33, 3, 896, True)])
def test_gru_xl_producer_splits(dev, t, n, h, bidir, monkeypatch):
    """Outputs and every gradient finite; a second run bit-identical (fixed summation order
    whatever the arrival order); every group forced GLOBAL (DS2_GRU_XL=2, sc1 stores)
    bit-identical to LOCAL; within 2e-5 of the fp32-MFMA kernels (DS2_GRU_X6=0)."""
    nd = 2 if bidir else 1
    env = [{"DS2_GRU_XL": "1", "DS2_GRU_X6": "1"}, {"DS2_GRU_XL": "1"}, {"DS2_GRU_XL": "2"},
           {"DS2_GRU_XL": "1", "DS2_GRU_X6": "0"}]
    loc, again, glob, f32 = _gru_run(dev, n, t, 40, h, nd, h + 7 * n, env, monkeypatch)
    for i, (a, b, c, d) in enumerate(zip(loc, again, glob, f32)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(a, b), f"output {i}: second run differs"
        assert torch.equal(a, c), f"output {i}: GLOBAL differs from LOCAL"
        _close(a, d, 2e-5, f"output {i}: XCD-local vs fp32 MFMA")


@pytest.mark.parametrize("n,h,bidir", [(32, 800, True), (13, 256, True), (7, 96, False)])
def test_gru_bwd_row_maxima(dev, n, h, bidir, monkeypatch):
    """The row maxima of dgx the XCD-local backward keeps (ds2_gru_row_amax): bit-equal to
    torch's amax of the dgx the layer handed to its GEMMs (ds2_amax's row format), 0 on the
    padded rows, and dX bit-identical to the one ds2_amax's rows give.  With DS2_GRU_XL=0 no
    partials exist: the layer gets no row_amax, takes the ds2_amax pass and still agrees."""
    nd = 2 if bidir else 1
    t = 29
    seen = {}
    orig = ops._rnn_param_grads

    def spy(x, h_all, dgx, dgh, weights, nd_, g, need_dx, bf16=False, pre=None, dbias=None, **kw):
        seen["dgx"], seen["row"] = dgx.clone(), kw.get("row_amax")
        out = orig(x, h_all, dgx, dgh, weights, nd_, g, need_dx, bf16, pre, dbias, **kw)
        if kw.get("row_amax") is not None:
            plain = dict(kw, row_amax=None)
            seen["dx_amax"] = orig(x, h_all, dgx, dgh, weights, nd_, g, need_dx, bf16, pre,
                                   dbias, **plain)[0].clone()
        seen["dx"] = out[0].clone()
        return out

    monkeypatch.setattr(ops, "_rnn_param_grads", spy)
    xl, = _gru_run(dev, n, t, 40, h, nd, h + n, [{"DS2_GRU_XL": "1"}], monkeypatch)
    row = seen["row"]
    assert row is not None and row.dtype == torch.int32 and row.shape == (t * n,)
    ref = seen["dgx"].view(t * n, -1).abs().amax(1).contiguous().view(torch.int32)
    assert torch.equal(row, ref)
    pad = (torch.arange(t).view(t, 1) >= _lens(t, n).view(1, n)).view(-1).to(dev)
    assert pad.any() and (row[pad] == 0).all()
    assert torch.equal(seen["dx"], seen["dx_amax"])
    seen.clear()
    plain, = _gru_run(dev, n, t, 40, h, nd, h + n, [{"DS2_GRU_XL": "0"}], monkeypatch)
    assert seen["row"] is None and "dx_amax" not in seen
    assert torch.isfinite(plain[1]).all()
    _close(plain[1], xl[1], 2e-5, "dX: 16-unit kernels + ds2_amax vs XCD-local + its row maxima")
