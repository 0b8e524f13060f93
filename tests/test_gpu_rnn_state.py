"""GPU: the forward recurrences from an initial state (ds2_gru_fwd_state, ds2_lstm_fwd_state;
ops.gru_forward_state, ops.lstm_forward_state) against float64 nn.GRU / nn.LSTM.

A sequence run in two chunks, the second from the state the first left, must equal the float64
module over the whole sequence at the layer tests' 1e-5 of max |ref| (check_close's bound for
y); so must one call from a given non-zero state.  Every case pins the rung and the table entry
through the launch record: the state must not change which kernel the shape selects.  The
shapes are one per forward rung of each ladder (DESIGN.md "Recurrent dispatch"), the rungs
behind an environment switch included, and the production widths whose instance key depends on
H.  layer_case and _close are test_gpu_rnn_ladder's.
"""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from ds2amd import _lib, ops
from test_gpu_rnn_ladder import _close, layer_case

pytestmark = pytest.mark.gpu

T, INP = 5, 12
SPLITS = [(2, 3), (1, 4), (4, 1)]

# (kind, n, h, environment switches) -> (rung, instance key); per_step launches once per step
RUNGS = {
    ("gru", 3, 32, ()): ("xcd_local", 2),
    ("gru", 3, 48, ()): ("h3_16", 1),
    ("gru", 3, 20, ()): ("lds_persist", 8),
    ("gru", 3, 6, ()): ("per_step", 8),
    ("gru", 3, 48, (("DS2_GRU_H3", "0"),)): ("x6_16", 1),      # the 16-unit bf16x6 kernels
    ("gru", 3, 48, (("DS2_GRU_X6", "0"),)): ("dop", 1),        # fp32-MFMA direct operand
    ("lstm", 3, 32, ()): ("dop_h3", 1),                        # h % 16 == 0
    ("lstm", 3, 20, ()): ("lds_persist", 8),                   # h % 4 == 0
    ("lstm", 3, 6, ()): ("per_step", 8),
    ("lstm", 3, 32, (("DS2_LSTM_H3", "0"),)): ("dop", 1),
    # production widths: the key follows H; n = 9 has a partial second sample tile
    ("gru", 1, 800, ()): ("xcd_local", 7),
    ("gru", 9, 800, ()): ("xcd_local", 7),
    ("lstm", 9, 1024, ()): ("dop_h3", 8),
}
SMALL = [k for k in RUNGS if k[2] < 400]
WIDE = [k for k in RUNGS if k[2] >= 400]


def ids(cases):
    return ["-".join([k, str(n), str(h)] + [f"{a}={b}" for a, b in env]) for k, n, h, env in cases]


def amp(kind, h):
    return h ** -0.5 if h > 400 else (0.3 if kind == "gru" else 0.1)


def make(kind, n, h, t=T, lens=None):
    """(float64 module, lens, x) with every sample full length unless lens is given"""
    if lens is None:
        lens = torch.full((n,), t, dtype=torch.int32)
    mod, lens, x, _ = layer_case(kind, n, h, d=1, t=t, inp=INP, amp=amp(kind, h), lens=lens)
    return mod, lens, x


def state64(kind, n, h, seed=5):
    """a random state of amplitude 0.5: (h0,) or (h0, c0), float64 [n, h]"""
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.rand(n, h, generator=g, dtype=torch.float64) * 2 - 1) * 0.5
                 for _ in range(1 if kind == "gru" else 2))


def ref64(kind, mod, x, lens, state=None):
    """pack -> float64 module (from `state`) -> pad: (y [t, n, h], final state tuple)"""
    hx = None
    if state is not None:
        hx = state[0][None] if kind == "gru" else (state[0][None], state[1][None])
    with torch.no_grad():
        out, fin = mod(pack_padded_sequence(x, lens.long(), enforce_sorted=False), hx)
    y, _ = pad_packed_sequence(out, total_length=x.shape[0])
    return y, ((fin[0],) if kind == "gru" else (fin[0][0], fin[1][0]))


def run(kind, dev, mod, x, lens, state=None):
    """ops.{gru,lstm}_forward_state on the device: (y, final state tuple, launch record)"""
    w = [p.detach().float().to(dev) for p in mod.parameters()]
    st = () if state is None else tuple(s.float().to(dev) for s in state)
    fn = ops.gru_forward_state if kind == "gru" else ops.lstm_forward_state
    with torch.no_grad():
        y, *fin = fn(x.float().to(dev), lens.to(dev), w, *st)
    rec = ops.rnn_last_launch()
    ops.check_rnn_status(dev)
    return y, tuple(fin), rec


def took(rec, case, steps):
    rung, k = RUNGS[case]
    want = (rung, k, steps if rung == "per_step" else 1)
    assert (rec.rung, rec.k, rec.launches) == want, f"launched {rec}, wanted {want}"


def setenv(monkeypatch, env):
    for name, value in env:
        monkeypatch.setenv(name, value)


def chunked(dev, case, t, split):
    """first part without a state, second from the state read from the first; the
    concatenation against float64 over all of t, and the rung in both calls"""
    kind, n, h, _ = case
    mod, lens, x = make(kind, n, h, t)
    ref, ref_fin = ref64(kind, mod, x, lens)
    a, b = split
    la, lb = torch.full((n,), a, dtype=torch.int32), torch.full((n,), b, dtype=torch.int32)
    y1, st, rec1 = run(kind, dev, mod, x[:a], la)
    took(rec1, case, a)
    y2, fin, rec2 = run(kind, dev, mod, x[a:], lb, tuple(s.double().cpu() for s in st))
    took(rec2, case, b)
    e = _close(torch.cat([y1, y2]), ref, 1e-5, f"{case} split {split} y")
    for got, want, name in zip(fin, ref_fin, "hc"):
        e = max(e, _close(got, want.reshape(n, h), 1e-5, f"{case} split {split} final {name}"))
    print(f"{case} split {split}: err/bound {e:.3f}")


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: f"{s[0]}+{s[1]}")
@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_chunked_equals_whole_fp64(dev, monkeypatch, case, split):
    setenv(monkeypatch, case[3])
    chunked(dev, case, T, split)


@pytest.mark.parametrize("case", WIDE, ids=ids(WIDE))
def test_chunked_production_widths(dev, case):
    """H 800 (GRU: 25 producers, 7 per wave) and 1024 (LSTM: 8 blocks per wave), T = 3 as 1 + 2"""
    chunked(dev, case, 3, (1, 2))


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_given_state_matches_fp64(dev, monkeypatch, case):
    """a random non-zero h0 (and c0) handed in directly, ragged lengths"""
    setenv(monkeypatch, case[3])
    kind, n, h, _ = case
    mod, lens, x = make(kind, n, h, lens=torch.tensor([T, T - 2, 1], dtype=torch.int32))
    st = state64(kind, n, h)
    ref, ref_fin = ref64(kind, mod, x, lens, st)
    y, fin, rec = run(kind, dev, mod, x, lens, st)
    took(rec, case, T)
    _close(y, ref, 1e-5, f"{case} y")
    for got, want, name in zip(fin, ref_fin, "hc"):
        _close(got, want.reshape(n, h), 1e-5, f"{case} final {name}")
    for i in range(n):
        assert not y[int(lens[i]):, i].any(), "outputs past len must be 0"


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_null_state_is_the_stateless_entry(dev, monkeypatch, case):
    """the state entry point without a state launches the stateless kernels: bit-equal output"""
    setenv(monkeypatch, case[3])
    kind, n, h, _ = case
    mod, lens, x = make(kind, n, h, lens=torch.tensor([T, T - 1, 2], dtype=torch.int32))
    y, fin, rec = run(kind, dev, mod, x, lens)
    took(rec, case, T)
    w = [p.detach().float().to(dev) for p in mod.parameters()]
    layer = ops.GRULayerFn if kind == "gru" else ops.LSTMLayerFn
    with torch.no_grad():
        want = layer.apply(x.float().to(dev), lens.to(dev), True, h, *w)
    took(ops.rnn_last_launch(), case, T)
    assert torch.equal(y, want)
    assert torch.equal(fin[0], torch.stack([want[int(lens[i]) - 1, i] for i in range(n)]))


BY_SHAPE = [c for c in SMALL if not c[3]]     # the rungs no environment switch stands before


@pytest.mark.parametrize("case", BY_SHAPE, ids=ids(BY_SHAPE))
def test_ragged_chunk_state_continues(dev, case):
    """lens < t_max inside both chunks: outputs past each len are zero, and the state read at
    len - 1 carries on -- sample i equals the float64 module over its own valid frames"""
    kind, n, h, _ = case
    mod, _, x = make(kind, n, h, 8)
    l1 = torch.tensor([4, 2, 1], dtype=torch.int32)
    l2 = torch.tensor([4, 3, 0], dtype=torch.int32)   # sample 2 gets nothing in chunk 2
    y1, st, _ = run(kind, dev, mod, x[:4], l1)
    y2, fin, _ = run(kind, dev, mod, x[4:], l2, tuple(s.double().cpu() for s in st))
    for i in range(n):
        a, b = int(l1[i]), int(l2[i])
        xi = torch.cat([x[:a, i], x[4:4 + b, i]])[:, None]
        ref, ref_fin = ref64(kind, mod, xi, torch.tensor([a + b]))
        got = torch.cat([y1[:a, i], y2[:b, i]])[:, None]
        _close(got, ref, 1e-5, f"{case} sample {i} y")
        for g_, want in zip(fin, ref_fin):
            _close(g_[i], want.reshape(h), 1e-5, f"{case} sample {i} final state")
        assert not y1[a:, i].any() and not y2[b:, i].any()


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_invalid_state_arguments(dev, kind):
    """a partial state set, or two directions with a state: the invalid-value status, and the
    launch record stays empty (nothing was launched)"""
    lib = _lib.load()
    n, h, t, g = 3, 32, 2, 3 if kind == "gru" else 4
    f = lambda *s: torch.zeros(*s, device=dev)
    xproj, w, b = f(t, n, 2, g * h), f(g * h, h), f(g * h)
    h_all, c_all, h0, hp = f(t, n, 2, h), f(t, n, 2, h), f(n, h), f(n, g * h)
    lens = torch.full((n,), t, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.size(f"ds2_{kind}_fwd_workspace_size", n, h, 2), dtype=torch.uint8,
                     device=dev)
    p = lambda x: None if x is None else x.data_ptr()

    def call(nd, state):
        outs = (p(h_all),) + ((p(c_all),) if kind == "lstm" else ())
        return getattr(lib, f"ds2_{kind}_fwd_state")(
            t, n, h, nd, p(xproj), p(w), p(w), p(b), p(b), p(lens), *outs, None,
            *[p(s) for s in state], None, p(ws), ws.numel(), None)

    full = (h0, hp) if kind == "gru" else (h0, h0, hp)
    bad = [(1, full[:i] + (None,) + full[i + 1:]) for i in range(len(full))] + [(2, full)]
    for nd, state in bad:
        assert call(1, (None,) * len(full)) == 0          # leaves a launch in the record
        assert ops.rnn_last_launch().launches == 1
        h_all.fill_(7.0)
        assert call(nd, state) == 1, (nd, state)          # DS2_INVALID_VALUE
        rec = ops.rnn_last_launch()
        assert (rec.rung, rec.launches) == ("none", 0), rec
        assert bool((h_all == 7.0).all())


def test_requires_grad_raises(dev):
    mod, lens, x = make("gru", 3, 32)
    w = [p.detach().float().to(dev) for p in mod.parameters()]
    xd = x.float().to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError):
        ops.gru_forward_state(xd, lens.to(dev), w)
