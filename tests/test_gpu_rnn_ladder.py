"""GPU: every rung of the recurrent fallback ladders, reached by shape alone (no environment
switch): a correctness net over the ladders' conditions.  Which kernel ran cannot be seen from
Python; the shapes are the ones each rung's condition selects (DESIGN.md "Recurrent dispatch").
"""
import pytest
import torch

from ds2amd import ops

pytestmark = pytest.mark.gpu

T, INP = 5, 12

# (n, h): the rung the shape selects
GRU_CASES = [(3, 32),    # XCD-local
             (72, 32),   # 18 XCD-local groups: it declines, the 16-unit kernels run
             (3, 48),    # h % 32 != 0: 16-unit
             (3, 20),    # h % 16 != 0: LDS-staged persistent
             (3, 6)]     # h % 4 != 0: one launch per step
LSTM_CASE = (144, 512)   # 9 sixteen-sample tiles: neither tile size fits one launch, 3 chunks


def _close(got, ref, rel, name):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


def ragged_lens(n):
    return torch.tensor(sorted([T] + [max(1, T - (i % 4) - 1) for i in range(n - 1)],
                               reverse=True), dtype=torch.int32)


def layer_case(kind, n, h):
    """(float64 CPU module, lens, x [T, n, INP] zero past each length, dy [T, n, h])."""
    g = torch.Generator().manual_seed(n * 100 + h)
    mod = {"gru": torch.nn.GRU, "lstm": torch.nn.LSTM, "rnn": torch.nn.RNN}[kind](
        INP, h, bidirectional=True).double()
    a = 0.3 if kind == "gru" else 0.1
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) * a)
    lens = ragged_lens(n)
    x = torch.randn(T, n, INP, generator=g, dtype=torch.float64)
    for i in range(n):
        x[int(lens[i]):, i] = 0
    dy = torch.randn(T, n, h, generator=g, dtype=torch.float64)
    return mod, lens, x, dy


def run_layer(fn, dev, mod, lens, x, dy, h):
    """[y, dx, dweights...] of one bidirectional layer (directions summed) on the GPU."""
    ws = [p.detach().float().to(dev).requires_grad_(True) for p in mod.parameters()]
    xd = x.float().to(dev).requires_grad_(True)
    y = fn.apply(xd, lens.to(dev), True, h, *ws)
    y.backward(dy.float().to(dev))
    torch.cuda.synchronize()
    return [y.detach().cpu(), xd.grad.cpu()] + [w.grad.cpu() for w in ws]


@pytest.mark.parametrize("n,h", GRU_CASES)
def test_gru_ladder_rung_matches_fp64(dev, n, h):
    """GRULayerFn forward and backward against nn.GRU in float64: y 1e-5, gradients 1e-4 of
    their max (test_gru_layer's tolerances)."""
    gru, lens, x, dy = layer_case("gru", n, h)
    xr = x.clone().requires_grad_(True)
    out, _ = gru(torch.nn.utils.rnn.pack_padded_sequence(xr, lens.numpy()))
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    summed = out.view(T, n, 2, h).sum(2)
    summed.backward(dy)
    got = run_layer(ops.GRULayerFn, dev, gru, lens, x, dy, h)
    _close(got[0], summed, 1e-5, "gru y")
    _close(got[1], xr.grad, 1e-4, "gru dx")
    for (name, p), gw in zip(gru.named_parameters(), got[2:]):
        _close(gw, p.grad, 1e-4, "gru " + name)


def test_lstm_chunked_persistent_equals_per_step(dev, monkeypatch):
    """The chunk loop with more than one chunk (forward and backward) against the per-step
    kernels (DS2_RNN_PERSISTENT=0), at test_lstm_persistent_equals_per_step's 1e-5."""
    n, h = LSTM_CASE
    lstm, lens, x, dy = layer_case("lstm", n, h)
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DS2_RNN_PERSISTENT", flag)
        outs.append(run_layer(ops.LSTMLayerFn, dev, lstm, lens, x, dy, h))
    for a, b in zip(*outs):
        _close(a, b, 1e-5, "lstm chunked persistent vs per-step")
