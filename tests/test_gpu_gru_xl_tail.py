"""GPU: the tail of a step of the XCD-local GRU recurrences (csrc/gru_xl.hip) -- what lies
between a step's last MFMA and its publish: the io waves' running row pointers, the hi + lo fold
of the waves' partials in the producing wave, the folded partials' LDS layout, the failure word
carried to the publish barrier, the publish itself.

Shapes chosen for what that code can get wrong: T = 1 (only the epilogue's store, no real step)
and T = 2 (one real step), where the running pointers start and finish; T = 6 in both
directions with lengths that include 1 and T (the forward's ring wraps past its 4 slots, the
reverse direction walks a negative stride, rows at and past a sample's length are zeros);
N = 9 and N = 5 (a sample tile with one or five owners of eight: absent samples pass through
the fold and the io stores); H = 32 (one producer: waves 1-3 hold no tile and contribute zero
partials), 64 and 288; the backward with and without the row-maximum workspace (the input's
gradient wanted or not) and with dy for one or both directions (sum_dirs); the forward without
a gate cache (torch.no_grad) and from an initial state.

_close is test_gpu_gru_xl_instances' measure, 2e-5 its bound against the fp32-MFMA kernels.
"""
import pytest
import torch

from ds2amd import ops

pytestmark = pytest.mark.gpu

INP = 24


def _close(got, ref, rel, name):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


def _lens(t, n):
    """ragged, sorted, the first sample full length and the last of length 1 (where t > 1)"""
    return torch.tensor(sorted([max(1, t - i * max(1, (t - 1) // max(1, n - 1))) for i in range(n - 1)]
                               + [1], reverse=True), dtype=torch.int32)


def _weights(h, nd, seed):
    g = torch.Generator().manual_seed(seed)
    a = h ** -0.5
    return g, [torch.rand(s, generator=g) * 2 * a - a for s in
               [(3 * h, INP), (3 * h, h), (3 * h,), (3 * h,)] * nd]


def _gru_run(dev, t, n, h, nd, sum_dirs, xgrad, env, monkeypatch):
    """One GRU layer forward + backward per environment in `env`: ([y, dx?, dW...], the
    forward's launch record) per run."""
    g, weights = _weights(h, nd, 100 * h + 10 * n + t)
    lens = _lens(t, n)
    x = torch.randn(t, n, INP, generator=g)
    dy = None
    outs = []
    for e in env:
        for k, v in e.items():
            monkeypatch.setenv(k, v)
        ws = [w.to(dev).requires_grad_(True) for w in weights]
        xd = x.to(dev).requires_grad_(xgrad)
        y = ops.GRULayerFn.apply(xd, lens.to(dev), sum_dirs, h, *ws)
        rec = ops.rnn_last_launch()
        if dy is None:   # [t, n, h], or [t, n, 2 h] for two directions kept apart
            dy = torch.randn(y.shape, generator=g)
        y.backward(dy.to(dev))
        torch.cuda.synchronize()
        ops.check_rnn_status(dev)
        outs.append(([y.detach().cpu()] + ([xd.grad.cpu()] if xgrad else []) +
                     [w.grad.cpu() for w in ws], rec))
    return lens, outs


ENV = [{"DS2_GRU_XL": "1", "DS2_GRU_X6": "1"}, {"DS2_GRU_XL": "1"}, {"DS2_GRU_XL": "2"},
       {"DS2_GRU_XL": "1", "DS2_GRU_X6": "0"}, {"DS2_GRU_XL": "0", "DS2_GRU_X6": "1"}]

# t, n, h, bidirectional, sum_dirs, input gradient wanted (the backward's ROWS instantiation)
CASES = [
    (1, 9, 64, True, True, True),
    (1, 5, 32, False, True, False),
    (2, 5, 32, True, False, True),
    (2, 9, 288, True, True, False),
    (6, 9, 288, True, True, True),
    (6, 5, 64, True, False, False),
    (6, 9, 32, False, True, True),
]


@pytest.mark.parametrize("t,n,h,bidir,sum_dirs,xgrad", CASES)
def test_gru_xl_tail(dev, t, n, h, bidir, sum_dirs, xgrad, monkeypatch):
    """Outputs and every gradient finite; a second run bit-identical; every group forced GLOBAL
    (DS2_GRU_XL=2) bit-identical; within 2e-5 of the fp32-MFMA kernels (DS2_GRU_X6=0); outputs
    past a sample's length zero; and the case did not pass on a fallback: the launch record
    names the XCD-local rung, and from T = 2 on -- T = 1 has no recurrent product, h_0 = 0, so
    every kernel computes the same bits there -- the 16-unit kernels (DS2_GRU_XL=0), whose sums
    run in another order, do not give the same bits."""
    nd = 2 if bidir else 1
    lens, runs = _gru_run(dev, t, n, h, nd, sum_dirs, xgrad, ENV, monkeypatch)
    (loc, rec), (again, _), (glob, rec_g), (f32, _), (u16, rec16) = runs
    assert rec.rung == "xcd_local" and rec_g.rung == "xcd_local", (rec, rec_g)
    assert rec16.rung != "xcd_local", rec16
    for i, (a, b, c, d) in enumerate(zip(loc, again, glob, f32)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(a, b), f"output {i}: second run differs"
        assert torch.equal(a, c), f"output {i}: GLOBAL differs from LOCAL"
        _close(a, d, 2e-5, f"output {i}: XCD-local vs fp32 MFMA")
    for i in range(n):
        assert not loc[0][int(lens[i]):, i].any(), "outputs past len must be 0"
    if t > 1:
        assert any(not torch.equal(a, e) for a, e in zip(loc, u16)), \
            "bit-identical to the 16-unit kernels"


@pytest.mark.parametrize("t,n,h,bidir", [(1, 5, 32, True), (6, 9, 288, True), (6, 5, 64, False)])
def test_gru_xl_tail_no_grad(dev, t, n, h, bidir, monkeypatch):
    """The forward without a gate cache (gates == nullptr: the io waves store h alone): the bits
    of the forward that keeps one, LOCAL and forced GLOBAL."""
    nd = 2 if bidir else 1
    g, weights = _weights(h, nd, 7 * h + n + t)
    lens = _lens(t, n).to(dev)
    x = torch.randn(t, n, INP, generator=g).to(dev)
    ws = [w.to(dev) for w in weights]
    monkeypatch.setenv("DS2_GRU_XL", "1")
    y = ops.GRULayerFn.apply(x, lens, True, h, *[w.clone().requires_grad_(True) for w in ws])
    outs = []
    for mode in ("1", "2"):
        monkeypatch.setenv("DS2_GRU_XL", mode)
        with torch.no_grad():
            outs.append(ops.GRULayerFn.apply(x, lens, True, h, *ws))
        assert ops.rnn_last_launch().rung == "xcd_local"
    torch.cuda.synchronize()
    ops.check_rnn_status(dev)
    assert torch.isfinite(y).all()
    for o in outs:
        assert torch.equal(o, y.detach())


@pytest.mark.parametrize("t,n,h", [(2, 5, 32), (7, 9, 288)])
def test_gru_xl_tail_state(dev, t, n, h, monkeypatch):
    """The initial-state entry (ops.gru_forward_state) from a non-zero h0: a sequence run as
    1 + (t - 1) steps, the second call from the state the first left, against the same sequence
    in one piece.  Both are within the layer tests' 1e-5 of float64, so within 2e-5 of each
    other; the second call again, and forced GLOBAL, are bit-identical."""
    g, weights = _weights(h, 1, 3 * h + n)
    ws = [w.to(dev) for w in weights]
    x = torch.randn(t, n, INP, generator=g).to(dev)
    monkeypatch.setenv("DS2_GRU_XL", "1")
    whole, _ = ops.gru_forward_state(x, t, ws)
    y1, h1 = ops.gru_forward_state(x[:1].contiguous(), 1, ws)
    h1 = h1.clone()
    assert h1.abs().max().item() > 0
    # ragged in the second call: lengths from t - 1 down to 1
    lens2 = torch.tensor(sorted([max(1, t - 1 - i) for i in range(n)], reverse=True),
                         dtype=torch.int32).to(dev)
    outs = []
    for mode in ("1", "1", "2"):
        monkeypatch.setenv("DS2_GRU_XL", mode)
        y2, _ = ops.gru_forward_state(x[1:].contiguous(), lens2, ws, h1)
        assert ops.rnn_last_launch().rung == "xcd_local"
        outs.append(y2)
    torch.cuda.synchronize()
    ops.check_rnn_status(dev)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ref = whole[1:].clone()
    for i in range(n):
        ref[int(lens2[i]):, i] = 0
        assert not outs[0][int(lens2[i]):, i].any(), "outputs past len must be 0"
    _close(outs[0], ref, 2e-5, "state run vs one piece")
    _close(y1, whole[:1], 2e-5, "first step")
