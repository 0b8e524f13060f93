"""GPU: every instance of the recurrent kernels' tables and the entry points' length edges,
against float64.

Each case (a) asserts through the launch record (ops.rnn_last_launch) that the forward and
the backward took the intended rung and table entry -- a declined shape would otherwise pass
on a fallback -- and (b) compares y, dx and every parameter gradient with pack ->
nn.{GRU,LSTM,RNN}.double() -> pad (-> direction sum) on the CPU at the layer tests' bounds:
y 1e-5, gradients 1e-4 of their max.  Weights are uniform in (-a, a) with the layer tests'
amplitudes (GRU 0.3, LSTM and RNN 0.1; H^-0.5 above H = 400).

Table keys (GW = BW = 8 waves, XW = 4; UB = H / 16 unit blocks):
  kRnnFwd / kGruFwdH3 <K>   K = ceil(ceil(UB / 2) / 4)          1..7  (H <= 896)
  kRnnBwd / kGruBwdH3 / kLstmBwd <K>   K = ceil(UB / 8)         1..8
  kFwdDop[H3][BTS - 1] <K>  smallest of 1, 2, 4, 8 >= ceil(UB / 8)
  kFwdPersist[BTS - 1] <K>  smallest of 8, 16, 25, 32 >= ceil(H / 32)
  kBwdPersist (k, c, BTS)   smallest (c, k) with c 32 k >= 4 H, k of 8, 16, 25, 32, 48, 64,
                            c of 1, 2; BTS = 2: (32, ceil(4 H / 1024), 2)
  kFwdStep <K>  smallest of 8, 16, 32 >= ceil(ceil(H / 4) / 8)
  kBwdStep <K>  smallest of 8, 16, 32, 64 >= ceil(min(H, 512) / 8)
"""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from ds2amd import _lib, model as dsm, ops
from test_gpu_rnn_ladder import (LAYER_FNS, _close, check_close, layer_case, ragged_lens,
                                 reference, run_layer)

pytestmark = pytest.mark.gpu

INP = 12


def amp(kind, h):
    return h ** -0.5 if h > 400 else (0.3 if kind == "gru" else 0.1)


def took(r, rung, k, launches=1, c=0, bts=None):
    """the launch record r names this rung, table entry and launch count"""
    got = (r.rung, r.k, r.c, r.launches) + ((r.bts,) if bts is not None else ())
    want = (rung, k, c, launches) + ((bts,) if bts is not None else ())
    assert got == want, f"launched {r}, wanted {want}"


def run_case(dev, kind, n, h, d, t, fwd, bwd, sum_dirs=True, lens=None, tweak=None, a=None):
    """One layer against float64; fwd / bwd: keyword arguments of took().  Returns (layer
    outputs, reference outputs, lens)."""
    mod, lens, x, dy = layer_case(kind, n, h, d, t, INP, a if a is not None else amp(kind, h),
                                  lens, sum_dirs)
    if tweak is not None:
        with torch.no_grad():
            tweak(mod)
    ref = reference(mod, lens, x, dy, sum_dirs)
    rec = {}
    got = run_layer(LAYER_FNS[kind], dev, mod, lens, x, dy, h, sum_dirs, rec)
    ops.check_rnn_status(dev)
    took(rec["fwd"], **fwd)
    took(rec["bwd"], **bwd)
    for g_ in got:
        assert torch.isfinite(g_).all()
    ey, eg = check_close(kind, mod, got, ref)
    print(f"{kind} n={n} h={h} d={d} t={t} fwd={tuple(rec['fwd'])} bwd={tuple(rec['bwd'])} "
          f"err/bound y {ey:.3f} grad {eg:.3f}")
    return got, ref, lens


# ---------------------------------------------------------------------------- instance sweep
# H_lo = 16 (8 (k - 1) + 1): the last wave holds one unit block (maximal predication);
# H_hi = 16 (8 k - 1): nearly full with an odd UB, the last 32-unit pair half empty.
# All have H % 32 = 16: the GRU takes the 16-unit kernels with no switch.
# (k, H, n, D, T)
SWEEP = [(k, 16 * (8 * (k - 1) + 1 if lo else 8 * k - 1), (3, 16, 17, 32)[(2 * k + lo) % 4],
          1 + (k + lo) % 2, 5 + (k + 2 * lo) % 5) for k in range(1, 8) for lo in (1, 0)]
SWEEP8 = [(8, 912, 17, 2, 6), (8, 1008, 32, 2, 5)]   # backward K = 8 (GRU, LSTM)
DOP_K = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}


@pytest.mark.parametrize("k,h,n,d,t", SWEEP)
def test_rnn_instance_sweep(dev, k, h, n, d, t):
    """Tanh RNN, one-gate fp16x3: kRnnFwd<k> and kRnnBwd<k> for k = 1..7 at H = 16, 112 (1),
    144, 240 (2), 272, 368 (3), 400, 496 (4), 528, 624 (5), 656, 752 (6), 784, 880 (7)."""
    run_case(dev, "rnn", n, h, d, t, dict(rung="h3_16", k=k), dict(rung="h3_16", k=k))


@pytest.mark.parametrize("h", [912, 1008])
def test_rnn_bwd8_unreachable(dev, h):
    """kRnnBwd<8> would need UB >= 57 (H >= 912), where the forward has no instance
    (kRnnFwd stops at 7, UB <= 56) and rnn_grid declines both directions of the pass: the
    per-step kernels of rnn.hip run, forward and backward."""
    run_case(dev, "rnn", 17, h, 2, 5, dict(rung="per_step", k=0, launches=5),
             dict(rung="per_step", k=0, launches=5))


@pytest.mark.parametrize("k,h,n,d,t", SWEEP + SWEEP8)
def test_gru_instance_sweep(dev, k, h, n, d, t):
    """GRU, 16-unit fp16x3: kGruFwdH3<k> and kGruBwdH3<k> at the sweep's H (k = 1..7), and
    kGruBwdH3<8> at H = 912, 1008, where the forward has no 16-unit instance and runs the
    fp32 direct-operand gru_fwd_dop_kernel<8>."""
    fwd = dict(rung="h3_16", k=k) if k < 8 else dict(rung="dop", k=8)
    run_case(dev, "gru", n, h, d, t, fwd, dict(rung="h3_16", k=k))


BWD_PERSIST = {16: (8, 1), 112: (16, 1), 144: (25, 1), 240: (32, 1), 272: (48, 1), 368: (48, 1),
               400: (64, 1), 496: (64, 1), 528: (48, 2), 624: (48, 2), 656: (48, 2),
               752: (48, 2), 784: (64, 2), 880: (64, 2), 912: (64, 2), 1008: (64, 2)}


@pytest.mark.parametrize("h3", ["1", "0"])
@pytest.mark.parametrize("k,h,n,d,t", SWEEP + SWEEP8)
def test_lstm_instance_sweep(dev, k, h, n, d, t, h3, monkeypatch):
    """LSTM at the sweep's H.  Default: the fp16x3 direct-operand forward kFwdDop[1][0]<1, 2,
    4, 8> (ceil(UB / 8) = k blocks per wave of the 1 (k = 1), 2 (2), 4 (3, 4) or 8 (5..8)
    built) and kLstmBwd<k>, k = 1..8.  DS2_LSTM_H3=0: the fp32-MFMA forward kFwdDop[0][0] at
    the same keys and the LDS-staged backward kBwdPersist (k, c, 1) of BWD_PERSIST."""
    monkeypatch.setenv("DS2_LSTM_H3", h3)
    if h3 == "1":
        fwd, bwd = dict(rung="dop_h3", k=DOP_K[k], bts=1), dict(rung="h3_16", k=k)
    else:
        kb, cb = BWD_PERSIST[h]
        fwd, bwd = dict(rung="dop", k=DOP_K[k], bts=1), dict(rung="lds_persist", k=kb, c=cb, bts=1)
    run_case(dev, "lstm", n, h, d, t, fwd, bwd)


# ---------------------------------------------------------------------------- LSTM rungs
# H % 4 = 0, H % 16 != 0: (H, forward K, backward (k, c))
LDS_CASES = [(20, 8, (8, 1)), (100, 8, (16, 1)), (180, 8, (25, 1)), (244, 8, (32, 1)),
             (340, 16, (48, 1)), (500, 16, (64, 1)), (700, 25, (48, 2)), (1000, 32, (64, 2)),
             (260, 16, (48, 1)), (516, 25, (48, 2)), (804, 32, (64, 2))]


@pytest.mark.parametrize("i,h,kf,kb", [(i,) + c for i, c in enumerate(LDS_CASES)])
def test_lstm_lds_staged(dev, i, h, kf, kb):
    """The LDS-staged persistent LSTM kernels by shape: kFwdPersist[0]<8, 16, 25, 32> and
    kBwdPersist (8..64, 1, 1), (48, 2, 1), (64, 2, 1)."""
    n, d, t = (3, 16, 17, 32)[i % 4], 1 + i % 2, 5 + i % 5
    run_case(dev, "lstm", n, h, d, t, dict(rung="lds_persist", k=kf, bts=1),
             dict(rung="lds_persist", k=kb[0], c=kb[1], bts=1))


# BTS = 2: 8 ceil(UB D / 8) BT > 256 >= 8 ceil(UB D / 8) ceil(BT / 2); T = 3, bidirectional, the
# last 32-sample workgroup half empty.  The LDS-staged backward keeps BTS = 2 up to H = 512 and
# runs in 16-sample chunks above.  (n, H, forward (rung, K), fp16x3 backward (K, launches),
# LDS-staged backward (k, c, BTS, launches))
BTS2_CASES = [(257, 128, ("dop", 1), (1, 2), (32, 1, 2, 1)),
              (129, 256, ("dop", 2), (2, 2), (32, 1, 2, 1)),
              (65, 400, ("dop", 4), (4, 2), (32, 2, 2, 1)),
              (49, 528, ("dop", 8), (5, 2), (48, 2, 1, 2)),
              (129, 244, ("lds_persist", 8), None, (32, 1, 2, 1)),
              (97, 260, ("lds_persist", 16), None, (32, 2, 2, 1)),
              (49, 516, ("lds_persist", 25), None, (48, 2, 1, 2)),
              (33, 804, ("lds_persist", 32), None, (64, 2, 1, 2))]


@pytest.mark.parametrize("h3", ["1", "0"])
@pytest.mark.parametrize("n,h,fw,kb3,kbp", BTS2_CASES)
def test_lstm_two_tiles_per_workgroup(dev, n, h, fw, kb3, kbp, h3, monkeypatch):
    """Two 16-sample tiles per workgroup in the forward, one launch: kFwdDop[.][1]<1, 2, 4, 8>
    (H % 16 = 0; fp16x3, or fp32 MFMA with DS2_LSTM_H3=0) and kFwdPersist[1]<8, 16, 25, 32>
    (H % 16 != 0, either setting).  Backward: the fp16x3 kLstmBwd<1, 2, 4, 5> in chunks of
    16 + 1, 8 + 1, 4 + 1, 3 + 1 tiles; LDS-staged (DS2_LSTM_H3=0, or H % 16 != 0) kBwdPersist
    (32, 1, 2) and (32, 2, 2) in one launch up to H = 512, (48, 2, 1) and (64, 2, 1) in two
    chunks above."""
    monkeypatch.setenv("DS2_LSTM_H3", h3)
    rung, kf = fw
    if rung == "dop" and h3 == "1":
        rung = "dop_h3"
    if h3 == "1" and kb3 is not None:
        bwd = dict(rung="h3_16", k=kb3[0], launches=kb3[1], bts=1)
    else:
        bwd = dict(rung="lds_persist", k=kbp[0], c=kbp[1], bts=kbp[2], launches=kbp[3])
    run_case(dev, "lstm", n, h, 2, 3, dict(rung=rung, k=kf, bts=2), bwd)


@pytest.mark.parametrize("h,kf,kb", [(6, 8, 8), (30, 8, 8), (126, 8, 16), (250, 8, 32),
                                     (510, 16, 64), (1022, 32, 64)])
def test_lstm_per_step_by_shape(dev, h, kf, kb):
    """H % 4 != 0: kFwdStep<8, 16, 32> and kBwdStep<8, 16, 32, 64>, one launch per step;
    H = 1022 stages the 4H gate columns in two chunks of 2048."""
    t = 5 + h % 3
    run_case(dev, "lstm", 17 if h < 200 else 3, h, 2, t, dict(rung="per_step", k=kf, launches=t),
             dict(rung="per_step", k=kb, launches=t))


@pytest.mark.parametrize("h", [6, 30, 126, 100])
def test_rnn_per_step_by_shape(dev, h):
    """H % 16 != 0: the tanh RNN's per-step kernels (rnn.hip; no instance table, key 0)."""
    t = 5 + h % 3
    run_case(dev, "rnn", 17, h, 2, t, dict(rung="per_step", k=0, launches=t),
             dict(rung="per_step", k=0, launches=t))


# ---------------------------------------------------------------------------- entry points
# one small H per rung family: (forward, backward) records, launches filled in by the case
def family(kind, h, t):
    if h % 4 != 0 or (kind == "rnn" and h % 16 != 0):
        k = 0 if kind == "rnn" else 8
        return dict(rung="per_step", k=k, launches=t), dict(rung="per_step", k=k, launches=t)
    if h % 16 != 0:
        return dict(rung="lds_persist", k=8), dict(rung="lds_persist", k=8, c=int(kind == "lstm"))
    fwd = dict(rung="dop_h3" if kind == "lstm" else "h3_16", k=1)
    return fwd, dict(rung="h3_16", k=1)


KINDS_H = [(kind, h) for kind in ("lstm", "rnn", "gru") for h in (16, 20, 6)]
T_EDGE = 7
EDGES = {   # name -> (t, lens)
    "unsorted": (T_EDGE, [3, 7, 1, 5, 7, 2, 6, 4, 1, 7, 5, 3, 6, 2, 4, 7, 1, 6, 3]),
    "short": (T_EDGE, [5, 4, 4, 2, 1]),          # max(lens) < T
    "t1": (1, [1, 1, 1]),
    "n1": (T_EDGE, [6]),
    "len1": (T_EDGE, [1] * 17),
    "full": (T_EDGE, [T_EDGE] * 17),
}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("kind,h", KINDS_H)
def test_length_edges_per_direction(dev, kind, h, edge):
    """sum_dirs=False (the per-direction output the drop-in modules use; dy_dirs = 2 in the
    backward) at the length edges, against pack_padded_sequence(enforce_sorted=False): lengths
    in no order over two batch tiles, max(lens) < T, T = 1, N = 1, every length 1, every length
    T.  Outputs and dx are exactly zero past each length."""
    t, lens = EDGES[edge]
    lens = torch.tensor(lens, dtype=torch.int32)
    fwd, bwd = family(kind, h, t)
    got, _, _ = run_case(dev, kind, len(lens), h, 2, t, fwd, bwd, sum_dirs=False, lens=lens)
    for i, ln in enumerate(lens.tolist()):
        assert (got[0][ln:, i] == 0).all() and (got[1][ln:, i] == 0).all()


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("kind,h", KINDS_H)
def test_unsorted_lengths_summed(dev, kind, h, d):
    """The direction sum with lengths in no order, one direction and two.  (One direction at
    H = 6: D H and D 3H are no multiples of 4, the per-step GRU and RNN backward run without
    the column maxima -- their layers used to fail there with DS2_UNSUPPORTED_SHAPE from the
    column pass after the recurrence.)"""
    t, lens = EDGES["unsorted"]
    fwd, bwd = family(kind, h, t)
    run_case(dev, kind, len(lens), h, d, t, fwd, bwd, lens=torch.tensor(lens, dtype=torch.int32))


@pytest.mark.parametrize("call", ["lengths", "no_lengths", "packed"])
@pytest.mark.parametrize("kind", ["lstm", "rnn", "gru"])
def test_module_matches_torch_module(dev, kind, call):
    """ds2amd.model.{LSTM,RNN,GRU} (per-direction output) against the torch module carrying
    the same state_dict in float64: forward(x, lengths) with unsorted lengths, forward(x)
    without lengths, PackedSequence in and out; output, dx and every parameter gradient."""
    n, h, t = 5, 16, 6
    lens = torch.tensor([t] * n if call == "no_lengths" else [3, 6, 1, 4, 6], dtype=torch.int32)
    ref_mod, lens, x, dy = layer_case(kind, n, h, 2, t, INP, amp(kind, h), lens, sum_dirs=False)
    ref = reference(ref_mod, lens, x, dy, sum_dirs=False)
    mod = {"lstm": dsm.LSTM, "rnn": dsm.RNN, "gru": dsm.GRU}[kind](INP, h, bidirectional=True)
    mod.load_state_dict({k: v.float() for k, v in ref_mod.state_dict().items()})
    mod = mod.to(dev)
    xd = x.float().to(dev).requires_grad_(True)
    rec = {}
    xd.register_hook(lambda _g: rec.__setitem__("bwd", ops.rnn_last_launch()))
    if call == "packed":
        out, _ = mod(pack_padded_sequence(xd, lens.long(), enforce_sorted=False))
        y, out_lens = pad_packed_sequence(out, total_length=t)
        assert out_lens.tolist() == lens.tolist()
    elif call == "lengths":
        y, _ = mod(xd, lens)
    else:
        y, _ = mod(xd)
    rec["fwd"] = ops.rnn_last_launch()
    y.backward(dy.float().to(dev))
    torch.cuda.synchronize()
    ops.check_rnn_status(dev)
    fwd, bwd = family(kind, h, t)
    took(rec["fwd"], **fwd)
    took(rec["bwd"], **bwd)
    got = [y.detach().cpu(), xd.grad.cpu()] + [dict(mod.named_parameters())[k].grad.cpu()
                                                for k, _ in ref_mod.named_parameters()]
    check_close(kind, ref_mod, got, ref)


INFER = [("gru", 32, "xcd_local", 2), ("gru", 16, "h3_16", 1), ("gru", 20, "lds_persist", 8),
         ("rnn", 16, "h3_16", 1), ("lstm", 16, "dop_h3", 1), ("lstm", 16, "dop", 1),
         ("lstm", 20, "lds_persist", 8)]


@pytest.mark.parametrize("kind,h,rung,k", INFER)
def test_inference_forward_bit_identical(dev, kind, h, rung, k, monkeypatch):
    """The torch.no_grad() forward (no gate cache, no c_all) is bit-identical to the training
    forward's y on every persistent rung."""
    monkeypatch.setenv("DS2_LSTM_H3", "0" if rung == "dop" else "1")
    n, t = 19, 7
    mod, lens, x, dy = layer_case(kind, n, h, 2, t, INP, amp(kind, h))
    rec = {}
    train = run_layer(LAYER_FNS[kind], dev, mod, lens, x, dy, h, True, rec)[0]
    took(rec["fwd"], rung, k)
    ws = [p.detach().float().to(dev) for p in mod.parameters()]
    with torch.no_grad():
        y = LAYER_FNS[kind].apply(x.float().to(dev), lens.to(dev), True, h, *ws)
    took(ops.rnn_last_launch(), rung, k)
    ops.check_rnn_status(dev)
    assert torch.equal(y.cpu(), train)
    _close(y, reference(mod, lens, x, dy)[0], 1e-5, kind + " y")


# ---------------------------------------------------------------------------- saturation
SAT = (12.0, -12.0, 50.0, -50.0, 200.0, -200.0)


def saturate(mod):
    """b_hh of six units per gate at +-12, +-50, +-200 (the units shifted by one from gate to
    gate), both directions: __expf underflows and overflows inside sigmoid_fast / tanh_fast.
    LSTM with H >= 16: unit 10 with i, f, o open and g = +1, unit 11 with g = -1: c = +-t after
    t steps."""
    h = mod.hidden_size
    gates = mod.bias_hh_l0.numel() // h
    for b in (mod.bias_hh_l0, mod.bias_hh_l0_reverse):
        for gi in range(gates):
            for j, v in enumerate(SAT):
                b[gi * h + (j + gi) % h] = v
        if gates == 4 and h >= 16:
            for u, gv in ((10, 50.0), (11, -50.0)):
                b[0 * h + u], b[1 * h + u], b[2 * h + u], b[3 * h + u] = 12.0, 12.0, gv, 12.0


@pytest.mark.parametrize("kind,h", [(kind, h) for kind in ("lstm", "rnn", "gru")
                                    for h in (16, 20, 22)] + [("gru", 32)])
def test_saturated_gates(dev, kind, h, monkeypatch):
    """Gate pre-activations at +-12, +-50 and +-200 and an LSTM cell state that grows past 10
    (T = 13): everything finite (no NaN from inf 0 or inf / inf) and within the usual bounds
    of float64, on the persistent rungs (16: fp16x3, 20: LDS-staged, GRU 32: XCD-local) and per
    step (22: H % 4 != 0 with units left unsaturated, so that max |y| stays of order 1 and the
    bounds, which are relative to it, keep their meaning: tanh_fast's absolute error is 1e-7)."""
    t = 13
    if (kind, h) == ("gru", 32):
        fwd = bwd = dict(rung="xcd_local", k=2)
    else:
        fwd, bwd = family(kind, h, t)
    lens = torch.tensor([13, 13, 12, 9, 4, 1, 13], dtype=torch.int32)
    got, ref, _ = run_case(dev, kind, len(lens), h, 2, t, fwd, bwd, lens=lens, tweak=saturate)
    if kind == "lstm" and h >= 16:
        assert ref[0].abs().max() > 0.99   # o tanh(c) with |c| up to 13: the state did grow


def test_lstm_saturated_fp32_mfma(dev, monkeypatch):
    """The same through the fp32-MFMA forward and the LDS-staged backward at H = 16."""
    monkeypatch.setenv("DS2_LSTM_H3", "0")
    lens = torch.tensor([13, 13, 12, 9, 4, 1, 13], dtype=torch.int32)
    run_case(dev, "lstm", len(lens), 16, 2, 13, dict(rung="dop", k=1),
             dict(rung="lds_persist", k=8, c=1), lens=lens, tweak=saturate)


# ---------------------------------------------------------------------------- W_hh row scales
def spread_rows(mod):
    """W_hh: row 0 all zero, row 1 of magnitude 1e-30, the others scaled by 10^U(-6, 0)."""
    g = torch.Generator().manual_seed(11)
    for w in (mod.weight_hh_l0, mod.weight_hh_l0_reverse):
        w.mul_(10 ** (-6 * torch.rand(w.shape[0], 1, generator=g, dtype=torch.float64)))
        w[0] = 0
        w[1] = torch.sign(w[1]) * 1e-30


@pytest.mark.parametrize("kind,h,fwd,bwd", [("gru", 16, ("h3_16", 1), ("h3_16", 1)),
                                            ("gru", 32, ("xcd_local", 2), ("xcd_local", 2)),
                                            ("rnn", 48, ("h3_16", 1), ("h3_16", 1)),
                                            ("lstm", 16, ("dop_h3", 1), ("h3_16", 1)),
                                            ("lstm", 144, ("dop_h3", 2), ("h3_16", 2))])
def test_w_hh_row_scales(dev, kind, h, fwd, bwd):
    """The fp16x3 recurrences scale each W_hh row by a power of two from its maximum: a zero
    row, a 1e-30 row and rows spread over six decades, at the usual bounds."""
    run_case(dev, kind, 19, h, 2, 7, dict(rung=fwd[0], k=fwd[1]), dict(rung=bwd[0], k=bwd[1]),
             tweak=spread_rows)


# ---------------------------------------------------------------------------- RNN col_amax
def rnn_fp64(xproj, w, b, lens, dy):
    """h and da = dL/d(pre-activation) of the tanh RNN in float64: xproj, dy [T, N, D, H]."""
    T, N, D, H = xproj.shape
    hs, da = torch.zeros_like(xproj), torch.zeros_like(xproj)
    for d in range(D):
        for i in range(N):
            steps = list(range(int(lens[i])))
            if d == 1:
                steps.reverse()
            hp = torch.zeros(H, dtype=torch.float64)
            for s in steps:
                hp = torch.tanh(xproj[s, i, d] + b[d] + w[d] @ hp)
                hs[s, i, d] = hp
            carry = torch.zeros(H, dtype=torch.float64)
            for s in reversed(steps):
                da[s, i, d] = (dy[s, i, d] + carry) * (1 - hs[s, i, d] ** 2)
                carry = w[d].T @ da[s, i, d]
    return hs, da


@pytest.mark.parametrize("n,h,rung,kf,kb", [(19, 48, "h3_16", 1, 1), (19, 272, "h3_16", 3, 3),
                                            (19, 30, "per_step", 0, 0)])
def test_rnn_bwd_column_maxima(dev, n, h, rung, kf, kb):
    """ds2_rnn_bwd_ws with a col_amax buffer: the column maxima of dg the fp16x3 weight-gradient
    GEMMs scale by, kept by the one-gate kernel as it runs or by ds2_amax after the per-step
    kernels: bit-exact against torch's column max of |dg| over [T N, D H]; h and dg within
    1e-5 / 1e-4 of the float64 recurrence."""
    t, nd = 7, 2
    g = torch.Generator().manual_seed(n + h)
    xproj = torch.randn(t, n, nd, h, generator=g) * 0.5
    a = amp("rnn", h)
    w = [(torch.rand(h, h, generator=g) * 2 - 1) * a for _ in range(nd)]
    b = [torch.rand(h, generator=g) * 0.2 - 0.1 for _ in range(nd)]
    dy = torch.randn(t, n, nd, h, generator=g)
    lens = ragged_lens(n, t)
    hs, da = rnn_fp64(xproj.double(), [x.double() for x in w], [x.double() for x in b], lens,
                      dy.double())
    xd, dyd, ld = xproj.to(dev), dy.to(dev), lens.to(dev)
    wd, bd = [x.to(dev) for x in w], [x.to(dev) for x in b]
    h_all = torch.full((t, n, nd, h), 7.0, device=dev)
    dg = torch.full((t, n, nd, h), 7.0, device=dev)
    col = torch.full((nd * h,), -1, dtype=torch.int32, device=dev)
    st = ops.rnn_status_word(dev)
    ws = ops._ws(_lib.size("ds2_rnn_fwd_workspace_size", n, h, nd), dev)
    _lib.call("ds2_rnn_fwd_ws", t, n, h, nd, xd.data_ptr(), wd[0].data_ptr(), wd[1].data_ptr(),
              bd[0].data_ptr(), bd[1].data_ptr(), ld.data_ptr(), h_all.data_ptr(), st.data_ptr(),
              ws.data_ptr(), ws.numel(), ops._stream())
    steps = t if rung == "per_step" else 1
    took(ops.rnn_last_launch(), rung, kf, steps)
    wsb = ops._ws(_lib.size("ds2_rnn_bwd_workspace_size", n, h, nd), dev)
    _lib.call("ds2_rnn_bwd_ws", t, n, h, nd, dyd.data_ptr(), nd, wd[0].data_ptr(),
              wd[1].data_ptr(), h_all.data_ptr(), ld.data_ptr(), dg.data_ptr(), col.data_ptr(),
              st.data_ptr(), wsb.data_ptr(), wsb.numel(), ops._stream())
    took(ops.rnn_last_launch(), rung, kb, steps)
    torch.cuda.synchronize()
    ops.check_rnn_status(dev)
    _close(h_all, hs, 1e-5, "rnn h")
    _close(dg, da, 1e-4, "rnn dg")
    want = dg.view(-1, nd * h).abs().amax(0).contiguous().view(torch.int32)
    assert torch.equal(col, want)
