"""GPU: every rung of the recurrent fallback ladders, reached by shape alone (no environment
switch): a correctness net over the ladders' conditions.  The shapes are the ones each rung's
condition selects (DESIGN.md "Recurrent dispatch"), and the launch record of the test hook
(ops.rnn_last_launch: rung, instance key, launches) pins that the rung named beside each case
is the one that ran, forward and backward.

layer_case / reference / run_layer / _close are shared with test_gpu_rnn_instances.py.
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
# ... as the launch record names it: (rung, forward instance key, backward instance key)
GRU_RUNGS = {(3, 32): ("xcd_local", 2, 2), (72, 32): ("h3_16", 1, 1), (3, 48): ("h3_16", 1, 1),
             (3, 20): ("lds_persist", 8, 8), (3, 6): ("per_step", 8, 8)}
LSTM_CASE = (144, 512)   # 9 sixteen-sample tiles: neither tile size fits one launch, 3 chunks

MODULES = {"gru": torch.nn.GRU, "lstm": torch.nn.LSTM, "rnn": torch.nn.RNN}
LAYER_FNS = {"gru": ops.GRULayerFn, "lstm": ops.LSTMLayerFn, "rnn": ops.RNNLayerFn}


def _close(got, ref, rel, name):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"
    return err / (rel * scale)


def ragged_lens(n, t=T):
    return torch.tensor(sorted([t] + [max(1, t - (i % 4) - 1) for i in range(n - 1)],
                               reverse=True), dtype=torch.int32)


def layer_case(kind, n, h, d=2, t=T, inp=INP, amp=None, lens=None, sum_dirs=True):
    """(float64 CPU module, lens, x [t, n, inp] zero past each length, dy [t, n, h], or
    [t, n, d h] per direction).  amp: the weights are uniform in (-amp, amp)."""
    g = torch.Generator().manual_seed(n * 100 + h)
    mod = MODULES[kind](inp, h, bidirectional=d == 2).double()
    a = amp if amp is not None else (0.3 if kind == "gru" else 0.1)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) * a)
    if lens is None:
        lens = ragged_lens(n, t)
    x = torch.randn(t, n, inp, generator=g, dtype=torch.float64)
    for i in range(n):
        x[int(lens[i]):, i] = 0
    dy = torch.randn(t, n, h if sum_dirs else d * h, generator=g, dtype=torch.float64)
    return mod, lens, x, dy


def reference(mod, lens, x, dy, sum_dirs=True):
    """[y, dx, dweights...] of pack -> the float64 module -> pad (-> direction sum) on the CPU;
    the lengths in any order."""
    t, n, _ = x.shape
    h, d = mod.hidden_size, 2 if mod.bidirectional else 1
    mod.zero_grad()
    xr = x.clone().requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(xr, lens.cpu().long(), enforce_sorted=False)
    out, _ = mod(packed)
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=t)
    if sum_dirs:
        out = out.view(t, n, d, h).sum(2)
    out.backward(dy)
    return [out.detach(), xr.grad] + [p.grad.clone() for p in mod.parameters()]


def run_layer(fn, dev, mod, lens, x, dy, h, sum_dirs=True, rec=None):
    """[y, dx, dweights...] of one layer (directions summed unless sum_dirs=False) on the GPU.
    rec (a dict): the launch records of the forward and of the backward, the latter read on
    autograd's worker thread, where the backward ran."""
    ws = [p.detach().float().to(dev).requires_grad_(True) for p in mod.parameters()]
    xd = x.float().to(dev).requires_grad_(True)
    y = fn.apply(xd, lens.to(dev), sum_dirs, h, *ws)
    if rec is not None:
        rec["fwd"] = ops.rnn_last_launch()
        xd.register_hook(lambda _g: rec.__setitem__("bwd", ops.rnn_last_launch()))
    y.backward(dy.float().to(dev))
    torch.cuda.synchronize()
    return [y.detach().cpu(), xd.grad.cpu()] + [w.grad.cpu() for w in ws]


def check_close(kind, mod, got, ref):
    """y at 1e-5, dx and every parameter gradient at 1e-4 of their max (test_gru_layer,
    test_lstm_layer, test_rnn_layer); returns the largest error / bound of (y, gradients)."""
    ey = _close(got[0], ref[0], 1e-5, kind + " y")
    eg = _close(got[1], ref[1], 1e-4, kind + " dx")
    for (name, _), gw, rw in zip(mod.named_parameters(), got[2:], ref[2:]):
        eg = max(eg, _close(gw, rw, 1e-4, kind + " " + name))
    return ey, eg


@pytest.mark.parametrize("n,h", GRU_CASES)
def test_gru_ladder_rung_matches_fp64(dev, n, h):
    """GRULayerFn forward and backward against nn.GRU in float64: y 1e-5, gradients 1e-4 of
    their max (test_gru_layer's tolerances); the rung and the instance are the case's."""
    gru, lens, x, dy = layer_case("gru", n, h)
    xr = x.clone().requires_grad_(True)
    out, _ = gru(torch.nn.utils.rnn.pack_padded_sequence(xr, lens.numpy()))
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    summed = out.view(T, n, 2, h).sum(2)
    summed.backward(dy)
    rec = {}
    got = run_layer(ops.GRULayerFn, dev, gru, lens, x, dy, h, rec=rec)
    rung, kf, kb = GRU_RUNGS[n, h]
    launches = T if rung == "per_step" else 1
    assert (rec["fwd"].rung, rec["fwd"].k, rec["fwd"].launches) == (rung, kf, launches), rec
    assert (rec["bwd"].rung, rec["bwd"].k, rec["bwd"].launches) == (rung, kb, launches), rec
    _close(got[0], summed, 1e-5, "gru y")
    _close(got[1], xr.grad, 1e-4, "gru dx")
    for (name, p), gw in zip(gru.named_parameters(), got[2:]):
        _close(gw, p.grad, 1e-4, "gru " + name)


def test_lstm_chunked_persistent_equals_per_step(dev, monkeypatch):
    """The chunk loop with more than one chunk (forward and backward) against the per-step
    kernels (DS2_RNN_PERSISTENT=0), at test_lstm_persistent_equals_per_step's 1e-5.  The
    persistent run is three launches of 4 + 4 + 1 tiles of kFwdDop<4> (fp16x3) and kLstmBwd<4>,
    the other T launches of kFwdStep<16> and kBwdStep<64>."""
    n, h = LSTM_CASE
    lstm, lens, x, dy = layer_case("lstm", n, h)
    outs = []
    want = {"1": (("dop_h3", 4, 3), ("h3_16", 4, 3)),
            "0": (("per_step", 16, T), ("per_step", 64, T))}
    for flag in ("1", "0"):
        monkeypatch.setenv("DS2_RNN_PERSISTENT", flag)
        rec = {}
        outs.append(run_layer(ops.LSTMLayerFn, dev, lstm, lens, x, dy, h, rec=rec))
        assert (rec["fwd"].rung, rec["fwd"].k, rec["fwd"].launches) == want[flag][0], rec
        assert (rec["bwd"].rung, rec["bwd"].k, rec["bwd"].launches) == want[flag][1], rec
    for a, b in zip(*outs):
        _close(a, b, 1e-5, "lstm chunked persistent vs per-step")
