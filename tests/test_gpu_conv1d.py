"""GPU: the Conv1d kernels (csrc/conv1d.hip) and the Wav2Letter pointwise kernels against
float64 torch on the CPU.  Activations are time-major on the device ([T, N, C]); the oracles
run on torch's [N, C, T]."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ds2amd import _lib, ops

pytestmark = pytest.mark.gpu


def _close(got, ref, rel=1e-5, name=""):
    """tests/test_gpu_ops.py's conv bound: max error <= rel * max |ref|."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    print(f"{name}: max err {err:.3e} ({err / scale:.2e} of max |ref| {scale:.3e})")
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"
    return err / scale


def _tnc(x_nct):
    return x_nct.permute(2, 0, 1).contiguous()


def _nct(x_tnc):
    return x_tnc.permute(1, 2, 0)


def _mode(monkeypatch, mode):
    if mode == "general":
        monkeypatch.setenv("DS2_CONV1D", "0")
    else:
        monkeypatch.delenv("DS2_CONV1D", raising=False)


@functools.lru_cache(maxsize=None)
def _case(t, n, ci, co, k, s, p, bias):
    """One float64 reference per shape, shared by both modes (never modified)."""
    g = torch.Generator().manual_seed(t + 3 * n + 5 * ci + 7 * co + 11 * k + 13 * s + 17 * p)
    x = torch.randn(n, ci, t, generator=g, dtype=torch.float64)
    w = torch.randn(co, ci, k, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(co, generator=g, dtype=torch.float64) if bias else None
    y = F.conv1d(x, w, b, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx = torch.nn.grad.conv1d_input(x.shape, w, dy, stride=s, padding=p)
    dw = torch.nn.grad.conv1d_weight(x, w.shape, dy, stride=s, padding=p)
    db = dy.sum((0, 2)) if bias else None
    return x, w, b, y, dy, dx, dw, db


def _run(dev, x, w, b, dy, s, p):
    xd, wd, dyd = _tnc(x).float().to(dev), w.float().to(dev), _tnc(dy).float().to(dev)
    bd = None if b is None else b.float().to(dev)
    y = ops.conv1d_fwd(xd, wd, bd, s, p)
    dx = ops.conv1d_dgrad(dyd, wd, tuple(xd.shape), s, p)
    dw, db = ops.conv1d_wgrad(dyd, xd, tuple(w.shape), s, p, with_bias=b is not None)
    return y, dx, dw, db


CASES = [
    # (T, N, Cin, Cout, k, s, p, bias)
    (37, 3, 161, 16, 13, 2, 6, False),     # the prolog: Cin % 4 != 0, stride 2, odd T
    (19, 2, 32, 64, 31, 1, 15, False),     # kernel longer than the sequence
    (3, 2, 32, 64, 31, 1, 15, False),      # every window clipped at both ends
    (19, 3, 24, 24, 1, 1, 0, True),        # the 1x1 block
    (19, 3, 24, 30, 1, 1, 0, True),        # the fc: Cout = 30 is not a tile multiple
    (140, 2, 32, 192, 13, 1, 6, False),    # more than one row tile and column tile
    (600, 4, 32, 32, 13, 1, 6, False),     # wgrad's long K = T N: split-K
    (20, 2, 8, 8, 4, 1, 2, False),         # even kernel, T_out = T + 1: general path
    (1, 1, 32, 32, 13, 1, 6, False),       # one row
]


@pytest.mark.parametrize("mode", ["fast", "general"])
@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "x".join(map(str, c[:7])))
def test_conv1d_parity(dev, cfg, mode, monkeypatch):
    """forward, dgrad, wgrad and dbias against float64, default and DS2_CONV1D=0."""
    t, n, ci, co, k, s, p, bias = cfg
    _mode(monkeypatch, mode)
    x, w, b, y, dy, dx, dw, db = _case(*cfg)
    yd, dxd, dwd, dbd = _run(dev, x, w, b, dy, s, p)
    assert tuple(yd.shape) == (y.shape[2], n, co)
    _close(_nct(yd), y, 1e-5, "conv1d fwd")
    _close(_nct(dxd), dx, 1e-5, "conv1d dgrad")
    _close(dwd, dw, 1e-5, "conv1d wgrad")
    if bias:
        _close(dbd, db, 1e-5, "conv1d dbias")


@pytest.mark.parametrize("mode", ["fast", "general"])
def test_conv1d_wgrad_is_deterministic(dev, mode, monkeypatch):
    """The split-K weight gradient sums its slabs in a fixed order: two runs, equal bits."""
    _mode(monkeypatch, mode)
    cfg = (600, 4, 32, 32, 13, 1, 6, False)
    x, w, b, y, dy, dx, dw, db = _case(*cfg)
    xd, dyd = _tnc(x).float().to(dev), _tnc(dy).float().to(dev)
    a, _ = ops.conv1d_wgrad(dyd, xd, tuple(w.shape), 1, 6, with_bias=False)
    c, _ = ops.conv1d_wgrad(dyd, xd, tuple(w.shape), 1, 6, with_bias=False)
    assert torch.equal(a, c)


def test_conv1d_fast_is_fp32_accurate(dev, monkeypatch):
    """Realistic K = 31 x 256 = 7936: both paths within 1e-5 of max |ref|, and the fp16x3
    path's error at most 2.5x the fp32 FMA path's (the form and factor of
    test_sgemm_x6_is_fp32_accurate / test_conv_x6_is_fp32_accurate)."""
    cfg = (64, 4, 256, 64, 31, 1, 15, False)
    x, w, b, y, dy, dx, dw, db = _case(*cfg)
    errs = {}
    for mode in ("fast", "general"):
        _mode(monkeypatch, mode)
        yd, dxd, dwd, _ = _run(dev, x, w, b, dy, 1, 15)
        errs[mode] = (_close(_nct(yd), y, 1e-5, f"{mode} fwd"),
                      _close(_nct(dxd), dx, 1e-5, f"{mode} dgrad"),
                      _close(dwd, dw, 1e-5, f"{mode} wgrad"))
    print("K=7936 relative errors", errs)
    assert all(f <= 2.5 * gen for f, gen in zip(errs["fast"], errs["general"])), errs


def test_conv1d_scales_over_twelve_decades(dev, monkeypatch):
    """test_conv_h3_scales_over_twelve_decades for Conv1d: samples and output channels of w
    spread over 10^+-6 (forward, dgrad), input and output channels spread likewise (wgrad).
    Error measured as max |y - y64| / (|w| conv |x|): the fast path within 2.5x of
    DS2_CONV1D=0's + 1e-7, and below 2e-6."""
    n, ci, t, co, k, s, p = 4, 32, 90, 32, 13, 1, 6
    g = torch.Generator().manual_seed(23)
    sx = torch.pow(10.0, torch.linspace(-6, 6, n, dtype=torch.float64))
    sw_ = torch.pow(10.0, torch.empty(co, dtype=torch.float64).uniform_(-6, 6, generator=g))
    x = torch.randn(n, ci, t, generator=g, dtype=torch.float64) * sx[:, None, None]
    wt = torch.randn(co, ci, k, generator=g, dtype=torch.float64) * 0.1 * sw_[:, None, None]
    y = F.conv1d(x, wt, None, stride=s, padding=p)
    yb = F.conv1d(x.abs(), wt.abs(), None, stride=s, padding=p)
    swi = torch.pow(10.0, torch.empty(ci, dtype=torch.float64).uniform_(-6, 6, generator=g))
    wt2 = torch.randn(co, ci, k, generator=g, dtype=torch.float64) * 0.1 * swi[None, :, None]
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64) * sx[:, None, None]
    dxr = torch.nn.grad.conv1d_input(x.shape, wt2, dy, stride=s, padding=p)
    dxb = torch.nn.grad.conv1d_input(x.shape, wt2.abs(), dy.abs(), stride=s, padding=p)
    xw = torch.randn(n, ci, t, generator=g, dtype=torch.float64) * swi[None, :, None]
    dyw = torch.randn(y.shape, generator=g, dtype=torch.float64) * sw_[None, :, None]
    dwr = torch.nn.grad.conv1d_weight(xw, wt.shape, dyw, stride=s, padding=p)
    dwb = torch.nn.grad.conv1d_weight(xw.abs(), wt.shape, dyw.abs(), stride=s, padding=p)
    errs = {}
    for mode in ("fast", "general"):
        _mode(monkeypatch, mode)
        yd = ops.conv1d_fwd(_tnc(x).float().to(dev), wt.float().to(dev), None, s, p)
        dx = ops.conv1d_dgrad(_tnc(dy).float().to(dev), wt2.float().to(dev), (t, n, ci), s, p)
        dwd, _ = ops.conv1d_wgrad(_tnc(dyw).float().to(dev), _tnc(xw).float().to(dev),
                                  tuple(wt.shape), s, p, with_bias=False)
        errs[mode] = tuple(((a.double().cpu() - r).abs() / b_.clamp_min(1e-300)).max().item()
                           for a, r, b_ in ((_nct(yd), y, yb), (_nct(dx), dxr, dxb),
                                            (dwd, dwr, dwb)))
    print("scale test errors", errs)
    assert all(f <= 2.5 * gen + 1e-7 for f, gen in zip(errs["fast"], errs["general"])), errs
    assert max(errs["fast"]) < 2e-6, errs


@pytest.mark.parametrize("c", [16, 25])
def test_glu_fwd_bwd(dev, c):
    rows = 57
    g = torch.Generator().manual_seed(c)
    x = (torch.randn(rows, 2 * c, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    y = F.glu(x, dim=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xd = x.detach().float().to(dev).requires_grad_(True)
    yd = ops.GLUFn.apply(xd)
    yd.backward(dy.float().to(dev))
    _close(yd, y, 1e-6, "glu fwd")
    _close(xd.grad, x.grad, 1e-6, "glu bwd")


@pytest.mark.parametrize("c", [16, 25])
def test_bn_relu_fwd_bwd(dev, c):
    """BatchNorm1d + ReLU in one pass and its backward against float64 F.batch_norm + relu;
    running statistics to 1e-5 (c = 25: odd, no float4 path)."""
    rows = 57
    g = torch.Generator().manual_seed(100 + c)
    x = torch.randn(rows, c, generator=g, dtype=torch.float64) * 3 + 1
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(c, generator=g, dtype=torch.float64)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    rm_d, rv_d = rm.float().to(dev), rv.float().to(dev)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.relu(F.batch_norm(xr, rm, rv, gr, br, training=True, momentum=0.1, eps=1e-5))
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xd = x.float().to(dev).requires_grad_(True)
    gd = gamma.float().to(dev).requires_grad_(True)
    bd = beta.float().to(dev).requires_grad_(True)
    yd = ops.BNReLUFn.apply(xd, gd, bd, rm_d, rv_d, True, 0.1, 1e-5)
    yd.backward(dy.float().to(dev))
    _close(yd, y, 1e-5, "bn_relu fwd")
    _close(xd.grad, xr.grad, 1e-5, "bn_relu dx")
    _close(gd.grad, gr.grad, 1e-5, "bn_relu dgamma")
    _close(bd.grad, br.grad, 1e-5, "bn_relu dbeta")
    _close(rm_d, rm, 1e-5, "running_mean")
    _close(rv_d, rv, 1e-5, "running_var")
    # eval mode: the running statistics
    ye = F.relu(F.batch_norm(x, rm, rv, gamma, beta, training=False, eps=1e-5))
    yed = ops.BNReLUFn.apply(x.float().to(dev), gd.detach(), bd.detach(), rm_d, rv_d, False, 0.1,
                             1e-5)
    _close(yed, ye, 1e-5, "bn_relu eval")


def test_bn_relu_leaves_the_next_conv_its_scales(dev):
    """BN + ReLU writes y's row / column maxima in the same pass (exact: they are maxima of
    the stored values), and a Conv1d given them computes what it computes on its own."""
    t, n, c = 23, 3, 32
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(t * n, c, generator=g) * 3 + 1).to(dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    y = ops.BNReLUFn.apply(x, gamma, beta, rm, rv, True, 0.1, 1e-5)
    y3 = y.view(t, n, c)
    w = (torch.randn(48, c, 13, generator=g) * 0.1).to(dev)
    dy = torch.randn(t, n, 48, generator=g).to(dev)
    rmax, cmax = ops._take_amax(y3, t * n, c)
    assert rmax is not None and cmax is not None
    assert torch.equal(rmax.view(torch.float32), y.abs().amax(1))
    assert torch.equal(cmax.view(torch.float32), y.abs().amax(0))
    assert torch.equal(ops.conv1d_fwd(y3, w, None, 1, 6, x_row_amax=rmax),
                       ops.conv1d_fwd(y3, w, None, 1, 6))
    a, _ = ops.conv1d_wgrad(dy, y3, tuple(w.shape), 1, 6, with_bias=False, x_col_amax=cmax)
    b, _ = ops.conv1d_wgrad(dy, y3, tuple(w.shape), 1, 6, with_bias=False)
    assert torch.equal(a, b)


def test_nct_to_tnc(dev):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 161, 37, generator=g)
    assert torch.equal(ops.nct_to_tnc(x.to(dev)).cpu(), x.permute(2, 0, 1).contiguous())


def test_conv1d_argument_checks(dev):
    """n == 0 is DS2_OK; negative sizes and T_out <= 0 are DS2_INVALID_VALUE; all of them
    return before any launch (NULL pointers throughout)."""
    lib = _lib.load()
    tail = (None, 0, None)
    assert lib.ds2_conv1d_fwd(None, None, None, None, 10, 0, 8, 8, 3, 1, 1, *tail) == 0
    assert lib.ds2_conv1d_fwd(None, None, None, None, 0, 2, 8, 8, 3, 1, 1, *tail) == 0
    assert lib.ds2_conv1d_dgrad(None, None, None, 10, 0, 8, 8, 3, 1, 1, *tail) == 0
    for bad in [(-1, 2, 8, 8, 3, 1, 1), (10, -2, 8, 8, 3, 1, 1), (10, 2, -8, 8, 3, 1, 1),
                (10, 2, 8, -8, 3, 1, 1), (10, 2, 8, 8, -3, 1, 1), (10, 2, 8, 8, 3, 0, 1),
                (10, 2, 8, 8, 3, 1, -1),
                (4, 2, 8, 8, 13, 1, 2)]:       # T + 2p - k < 0: T_out <= 0
        assert lib.ds2_conv1d_fwd(None, None, None, None, *bad, *tail) == 1, bad
        assert lib.ds2_conv1d_dgrad(None, None, None, *bad, *tail) == 1, bad
        assert lib.ds2_conv1d_wgrad(None, None, None, None, *bad, *tail) == 1, bad
    torch.cuda.synchronize()
