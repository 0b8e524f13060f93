"""GPU: the fused Adam and decayed SGD-Nesterov updates (ds2_clip_adam,
ds2_clip_sgd_nesterov_wd; FusedAdam, FusedSGD(weight_decay), Trainer(optimizer='adam')).

Arbiter: torch.optim.Adam / SGD in float64 on the CPU.  Yardstick: the same torch optimizer
in float32.  After every step, for each of p, exp_avg and exp_avg_sq over the whole tensor,

    max|ours - fp64|  <=  2 * max|torch_fp32 - fp64|  +  2^-24 * max|fp64|

(the factor 2 allows an equally valid fp32 operation order, the last term half an ulp of the
largest element).  Adam's update is ill-conditioned where |g'| <~ eps and a clip coefficient
of another precision rescales every g', so the inputs keep the reference alone inside the
bound: all three optimizers get the SAME fp32 clipped gradients (the raw ones times the
coefficient formed, in fp32 like the kernel, from the device's own norm read back; that norm
is checked on its own against the float64 norm at 1e-6); gradient magnitudes are log-uniform
in [1e-3, 1] with random signs, |p| in [0.5, 2] * lr, every 7th gradient exactly 0 in the
weight_decay = 0 cases only, and with decay the test asserts min|g coef| >= 4 wd max|p|.

Each check prints its figures (run with -s to see them).  On an MI355X the kernel, which
keeps ATen's operation order, had exactly torch-fp32's max error in 148 of the 177 checks and
at worst 0.79 of the bound (n = 3, step 3, p).
"""
import os

import numpy as np
import pytest
import torch

from ds2amd import _lib, ops
from ds2amd import model as dsm
from ds2amd.optim import FlatParams, FusedAdam, FusedSGD
from ds2amd.trainer import Trainer
from oracle import ds2_oracle as orc

pytestmark = pytest.mark.gpu

LABELS = orc.LABELS
CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
BETAS, EPS = (0.9, 0.999), 1e-8
WDS = [0.0, 1e-4]


# ------------------------------------------------------------------ inputs and the bound
def _signs(g, n):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def _params(g, n, lr):
    return ((0.5 + 1.5 * torch.rand(n, generator=g)) * lr * _signs(g, n)).float()


def _grads(g, n, zeros, scale=1.0):
    x = (10.0 ** (-3.0 * torch.rand(n, generator=g)) * _signs(g, n) * scale).float()
    if zeros:
        x[3::7] = 0.0
    return x


def _within_bound(what, ours, t32, t64):
    ours, t32 = ours.detach().double().cpu().reshape(-1), t32.detach().double().reshape(-1)
    t64 = t64.detach().reshape(-1)
    e_ours = (ours - t64).abs().max().item()
    e_t32 = (t32 - t64).abs().max().item()
    bound = 2.0 * e_t32 + 2.0 ** -24 * t64.abs().max().item()
    print(f"{what}: ours {e_ours:.3e} torch-fp32 {e_t32:.3e} bound {bound:.3e}")
    assert e_ours <= bound, f"{what}: max|ours-fp64| {e_ours:.3e} > {bound:.3e} " \
                            f"(torch fp32 {e_t32:.3e})"


def _clip_coef(norm32: float, max_norm: float) -> float:
    """min(1, max_norm / (norm + 1e-6)) in fp32, as the kernels (and clip_grad_norm_) form it."""
    c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return float(min(c, np.float32(1.0)))


def _check_norm(norm32: float, grads):
    ref = torch.cat([x.reshape(-1) for x in grads]).double().norm().item()
    assert abs(norm32 - ref) <= 1e-6 * ref, (norm32, ref)


def _check_decay_dominated(gc, wd, p64):
    if wd > 0:
        least, most = gc.abs().min().item(), p64.abs().max().item()
        assert least >= 4 * wd * most, (least, most)


class _TorchPair:
    """torch.optim.Adam in float32 (yardstick) and float64 (arbiter) on one flat tensor."""

    def __init__(self, p0, lr, wd, state=None):
        self.p32 = torch.nn.Parameter(p0.clone().float())
        self.p64 = torch.nn.Parameter(p0.clone().double())
        self.o32 = torch.optim.Adam([self.p32], lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
        self.o64 = torch.optim.Adam([self.p64], lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
        if state is not None:
            t, m, v = state
            for o, dt in ((self.o32, torch.float32), (self.o64, torch.float64)):
                sd = o.state_dict()
                sd['state'] = {0: {'step': torch.tensor(float(t)), 'exp_avg': m.to(dt).clone(),
                                   'exp_avg_sq': v.to(dt).clone()}}
                o.load_state_dict(sd)

    def step(self, gc):
        self.p32.grad = gc.clone()
        self.p64.grad = gc.double()
        self.o32.step()
        self.o64.step()

    def check(self, what, p, m, v):
        s32, s64 = self.o32.state[self.p32], self.o64.state[self.p64]
        _within_bound(what + " p", p, self.p32, self.p64)
        _within_bound(what + " exp_avg", m, s32['exp_avg'], s64['exp_avg'])
        _within_bound(what + " exp_avg_sq", v, s32['exp_avg_sq'], s64['exp_avg_sq'])


class _RawAdam:
    """ds2_clip_adam and ds2_grad_norm on plain device buffers."""

    def __init__(self, dev, p0, lr, wd, t0=0, m0=None, v0=None):
        self.dev, self.lr, self.wd, self.n = dev, lr, wd, p0.numel()
        self.p = p0.clone().to(dev)
        self.m = torch.zeros_like(self.p) if m0 is None else m0.clone().to(dev)
        self.v = torch.zeros_like(self.p) if v0 is None else v0.clone().to(dev)
        self.g = torch.zeros_like(self.p)
        self.count = torch.full((1,), t0, dtype=torch.int32, device=dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.ws = torch.empty(max(16, _lib.size("ds2_optim_workspace_size", self.n)),
                              dtype=torch.uint8, device=dev)

    def grad_norm(self, grads) -> float:
        self.g.copy_(grads)
        _lib.call("ds2_grad_norm", self.g.data_ptr(), self.n, self.norm.data_ptr(),
                  self.ws.data_ptr(), self.ws.numel(), ops._stream())
        return float(self.norm.item())

    def step(self, grads, max_norm, use_norm=True, skip=None):
        self.g.copy_(grads)
        _lib.call("ds2_clip_adam", self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(),
                  self.v.data_ptr(), self.n, self.lr, BETAS[0], BETAS[1], EPS, self.wd,
                  max_norm, self.norm.data_ptr() if use_norm else None, self.count.data_ptr(),
                  None if skip is None else skip.data_ptr(), ops._stream())


# ------------------------------------------------------------------ 1. raw sizes
# 2048 * 256 * 4 + 1027: the float4 grid-stride loop goes round a second time (grid cap 2048
# blocks x 256 threads x 4 floats) and the scalar tail (numel % 4 = 3) runs.
SIZES = [1, 3, 4, 5, 1027, 2048 * 256 * 4 + 1027]


@pytest.mark.parametrize("wd", WDS)
@pytest.mark.parametrize("numel", SIZES)
def test_clip_adam_sizes_four_steps(dev, numel, wd):
    """Four steps of the raw entry point: max_norm = 1 (steps 1 and 4), gradients x50 so the
    clip bites hard (step 2), norm = NULL (step 3).  The device counter reads 4 at the end."""
    lr = 1e-4
    g = torch.Generator().manual_seed(100 + numel % 1000)
    p0 = _params(g, numel, lr)
    raw = _RawAdam(dev, p0, lr, wd)
    ref = _TorchPair(p0, lr, wd)
    for step in range(4):
        grads = _grads(g, numel, zeros=(wd == 0), scale=50.0 if step == 1 else 1.0)
        coef = 1.0
        if step != 2:
            norm = raw.grad_norm(grads)
            _check_norm(norm, [grads])
            coef = _clip_coef(norm, 1.0)
            if step == 1 and numel >= 1027:
                assert coef < 0.05
        gc = grads * coef
        _check_decay_dominated(gc, wd, ref.p64.detach())
        raw.step(grads, 1.0, use_norm=(step != 2))
        ref.step(gc)
        ref.check(f"n={numel} wd={wd} step {step + 1}", raw.p, raw.m, raw.v)
        assert int(raw.count.item()) == step + 1
    assert int(raw.count.item()) == 4


# ------------------------------------------------------------------ 2. large t
@pytest.mark.parametrize("wd", WDS)
def test_clip_adam_bias_correction_at_step_1000(dev, wd):
    """Counter preset to 999 with non-zero moments, one step at lr = 1e-2: 1 - beta2^1000 =
    0.632 and lr / (1 - beta1^1000) must be the double-precision values rounded once (a float
    powf is off by ~1e-5 relative here, far outside the bound)."""
    n, lr = 1027, 1e-2
    g = torch.Generator().manual_seed(7)
    p0 = _params(g, n, lr)
    m0 = 0.5 * _grads(g, n, zeros=False)
    v0 = _grads(g, n, zeros=False) ** 2
    grads = _grads(g, n, zeros=(wd == 0))
    raw = _RawAdam(dev, p0, lr, wd, t0=999, m0=m0, v0=v0)
    ref = _TorchPair(p0, lr, wd, state=(999, m0, v0))
    norm = raw.grad_norm(grads)
    _check_norm(norm, [grads])
    gc = grads * _clip_coef(norm, 1.0)
    _check_decay_dominated(gc, wd, ref.p64.detach())
    raw.step(grads, 1.0)
    ref.step(gc)
    assert float(ref.o32.state[ref.p32]['step']) == 1000.0
    ref.check(f"t=1000 wd={wd}", raw.p, raw.m, raw.v)
    assert int(raw.count.item()) == 1000


# ------------------------------------------------------------------ 3. skip
def test_clip_adam_skip_leaves_everything_unchanged(dev):
    """A non-zero skip flag: p, both moments and the counter are bit-unchanged (on a fresh
    state and on a used one); the next unskipped step is torch's FIRST step."""
    n, lr = 1027, 1e-3
    g = torch.Generator().manual_seed(8)
    p0 = _params(g, n, lr)
    raw = _RawAdam(dev, p0, lr, 0.0)
    ref = _TorchPair(p0, lr, 0.0)
    on = torch.full((1,), 3, dtype=torch.int32, device=dev)
    off = torch.zeros(1, dtype=torch.int32, device=dev)
    grads = _grads(g, n, zeros=True)
    norm = raw.grad_norm(grads)
    raw.step(grads, 1.0, skip=on)
    assert torch.equal(raw.p.cpu(), p0)
    assert not raw.m.any().item() and not raw.v.any().item()
    assert int(raw.count.item()) == 0
    raw.step(grads, 1.0, skip=off)
    ref.step(grads * _clip_coef(norm, 1.0))
    ref.check("first step after a skipped one", raw.p, raw.m, raw.v)
    assert int(raw.count.item()) == 1
    before = [t.clone() for t in (raw.p, raw.m, raw.v)]
    raw.grad_norm(50.0 * grads)
    raw.step(50.0 * grads, 1.0, skip=on)
    for now, was in zip((raw.p, raw.m, raw.v), before):
        assert torch.equal(now.view(torch.int32), was.view(torch.int32))
    assert int(raw.count.item()) == 1


# ------------------------------------------------------------------ 4. FusedAdam / FlatParams
SHAPES = [(30, 7), (13,), (5, 5, 3), (1,)]


def _padding_mask(flat):
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for _, o, n in flat.slices():
        pad[o:o + n] = False
    return pad


def _model_order_vector(flat, buf):
    return torch.cat([buf[flat.offset_of[id(p)]:flat.offset_of[id(p)] + p.numel()]
                      for p in flat.model_params]).cpu()


@pytest.mark.parametrize("wd", WDS)
def test_fused_adam_matches_torch_and_resumes(dev, wd):
    """FusedAdam over ragged parameters: three steps against torch.optim.Adam; the alignment
    padding of the parameters and of both moments stays exactly 0; a fresh FusedAdam loaded
    from state_dict() then takes the same fourth step bit for bit."""
    lr = 1e-3
    g = torch.Generator().manual_seed(4)
    sizes = [int(np.prod(s)) for s in SHAPES]
    p0 = _params(g, sum(sizes), lr)
    init = [t.reshape(s) for t, s in zip(p0.split(sizes), SHAPES)]
    mine = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    flat = FlatParams(mine, dev)
    opt = FusedAdam(flat, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, max_norm=1.0)
    ref = _TorchPair(p0, lr, wd)        # Adam is elementwise: one flat tensor, model order
    pad = _padding_mask(flat)
    assert pad.sum().item() == flat.numel - sum(sizes) > 0

    def give(grads):
        opt.zero_grad()
        assert all(p.grad is None for p in mine)
        for p, gr, s in zip(mine, grads.split(sizes), SHAPES):
            p.grad = gr.reshape(s).to(dev)

    for step in range(3):
        grads = _grads(g, sum(sizes), zeros=(wd == 0), scale=50.0 if step == 1 else 1.0)
        give(grads)
        opt.step()
        norm = float(opt.norm.item())
        _check_norm(norm, [grads])
        gc = grads * _clip_coef(norm, 1.0)
        _check_decay_dominated(gc, wd, ref.p64.detach())
        ref.step(gc)
        ref.check(f"FusedAdam wd={wd} step {step + 1}", _model_order_vector(flat, flat.flat),
                  _model_order_vector(flat, opt.exp_avg), _model_order_vector(flat, opt.exp_avg_sq))
        for name, buf in (("flat", flat.flat), ("exp_avg", opt.exp_avg),
                          ("exp_avg_sq", opt.exp_avg_sq)):
            assert not buf.cpu()[pad].any().item(), f"{name} padding written at step {step + 1}"
    assert int(opt.step_count.item()) == 3

    # resume: state_dict -> a fresh FusedAdam over a copy of the parameters -> the same step
    sd = opt.state_dict()
    assert float(sd['state'][0]['step']) == 3.0 and sd['state'][0]['step'].dtype == torch.float32
    again = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    flat2 = FlatParams(again, dev)
    opt2 = FusedAdam(flat2, lr=123.0, max_norm=1.0)
    opt2.load_state_dict(sd)
    assert torch.equal(flat2.flat, flat.flat)
    grads = _grads(g, sum(sizes), zeros=(wd == 0))
    give(grads)
    for p, gr, s in zip(again, grads.split(sizes), SHAPES):
        p.grad = gr.reshape(s).to(dev)
    opt.step()
    opt2.step()
    assert int(opt.step_count.item()) == int(opt2.step_count.item()) == 4
    for name, a, b in (("flat", flat.flat, flat2.flat), ("exp_avg", opt.exp_avg, opt2.exp_avg),
                       ("exp_avg_sq", opt.exp_avg_sq, opt2.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


# ------------------------------------------------------------------ 5. SGD with weight decay
def _close(got, ref, tol, what):
    ref = ref.detach().double()
    err = (got.detach().double().cpu() - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-30)
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


def test_fused_sgd_weight_decay_matches_torch(dev):
    """FusedSGD(weight_decay=1e-4) (ds2_clip_sgd_nesterov_wd) against clip_grad_norm_ +
    torch.optim.SGD(nesterov=True, weight_decay=1e-4): three steps, the second one clipped,
    1e-6 of max|ref| as for the decay-free kernel (test_fused_sgd_matches_torch)."""
    g = torch.Generator().manual_seed(4)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    opt = torch.optim.SGD(ref, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    mine = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    flat = FlatParams(mine, dev)
    fopt = FusedSGD(flat, lr=0.01, momentum=0.9, max_norm=1.0, weight_decay=1e-4)
    pad = _padding_mask(flat)
    for step in range(3):
        grads = [torch.randn(s, generator=g) * (3 if step == 1 else 0.1) for s in SHAPES]
        for p, gr in zip(ref, grads):
            p.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(ref, 1.0)
        opt.step()
        fopt.zero_grad()
        for p, gr in zip(mine, grads):
            p.grad = gr.to(dev)
        fopt.step()
        for i, (p, r) in enumerate(zip(mine, ref)):
            _close(p, r, 1e-6, f"sgd wd step {step} param {i}")
            o = flat.offset_of[id(p)]
            _close(fopt.buf[o:o + p.numel()].view_as(p), opt.state[r]['momentum_buffer'], 1e-6,
                   f"sgd wd step {step} momentum {i}")
        assert not flat.flat.cpu()[pad].any().item() and not fopt.buf.cpu()[pad].any().item()


@pytest.mark.parametrize("numel", [5, 2048 * 256 * 4 + 1027])
def test_clip_sgd_nesterov_wd_raw_sizes(dev, numel):
    """The raw decayed-SGD entry at sizes with a scalar tail and a second trip of the float4
    loop, against float64 torch SGD on the same fp32 clipped gradients; a skipped call
    changes nothing."""
    lr, mom, wd = 0.01, 0.9, 1e-4
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(numel, generator=g)
    p = p0.clone().to(dev)
    buf = torch.zeros_like(p)
    norm = torch.zeros(1, dtype=torch.float32, device=dev)
    ws = torch.empty(max(16, _lib.size("ds2_optim_workspace_size", numel)), dtype=torch.uint8,
                     device=dev)
    r = torch.nn.Parameter(p0.double())
    opt = torch.optim.SGD([r], lr=lr, momentum=mom, nesterov=True, weight_decay=wd)
    on = torch.ones(1, dtype=torch.int32, device=dev)
    for step in range(2):
        grads = torch.randn(numel, generator=g)
        gd = grads.to(dev)
        _lib.call("ds2_grad_norm", gd.data_ptr(), numel, norm.data_ptr(), ws.data_ptr(),
                  ws.numel(), ops._stream())
        nv = float(norm.item())
        _check_norm(nv, [grads])
        args = [p.data_ptr(), gd.data_ptr(), buf.data_ptr(), numel, lr, mom, wd, 1.0,
                norm.data_ptr()]
        before = (p.clone(), buf.clone())
        _lib.call("ds2_clip_sgd_nesterov_wd", *args, on.data_ptr(), ops._stream())
        assert torch.equal(p, before[0]) and torch.equal(buf, before[1])
        _lib.call("ds2_clip_sgd_nesterov_wd", *args, None, ops._stream())
        r.grad = (grads * _clip_coef(nv, 1.0)).double()
        opt.step()
        _close(p, r, 1e-6, f"raw sgd wd n={numel} step {step}")
        _close(buf, opt.state[r]['momentum_buffer'], 1e-6, f"raw sgd wd n={numel} momentum {step}")


# ------------------------------------------------------------------ 6. Trainer
def test_trainer_adam_two_steps_and_checkpoint(dev, golden_dir):
    """Trainer(optimizer='adam') on the tiny golden model, two train_batch steps.  Each step is
    replayed on the CPU by float64 and float32 torch Adam from what the step itself used (the
    parameters before it, flat.grad, optimizer.norm) under the bound above: the wiring --
    zero_grad, the gradient slots, the device norm, the skip word, the step count -- without
    an Adam oracle.  Then serialize -> load_model_package -> a new Trainer ->
    load_state_dict restores the step count and both moments."""
    gd = np.load(os.path.join(golden_dir, 'tiny_ds2.npz'))
    torch.manual_seed(int(gd['seed']))
    model = dsm.DeepSpeech(rnn_type='gru', labels=LABELS, rnn_hidden_size=16, nb_layers=2,
                           audio_conf=CONF, bidirectional=True)
    # no decay here: real gradients hold zeros and tiny values, so the decay could not be kept
    # from dominating g' (module docstring); the decay's arithmetic is pinned by the cases above
    lr, wd, max_norm = 1e-3, 0.0, 100.0
    tr = Trainer(model, LABELS, lr=lr, max_norm=max_norm, device=dev, verbose=False,
                 optimizer='adam', weight_decay=wd, betas=BETAS, eps=EPS)
    assert isinstance(tr.optimizer, FusedAdam)
    n = tr.flat.numel
    ref = None
    for step in range(2):
        data = (torch.from_numpy(gd['x']), torch.from_numpy(gd['targets']), None,
                torch.from_numpy(gd['pct']).clone(), torch.from_numpy(gd['target_sizes']))
        pre = tr.flat.flat.detach().cpu().clone()
        loss = tr.train_batch(data, return_item=True)
        assert np.isfinite(loss)
        grads = tr.flat.grad[:n].detach().cpu().clone()
        assert grads.abs().max().item() > 0
        norm = float(tr.optimizer.norm.item())
        _check_norm(norm, [grads])
        if ref is None:
            ref = _TorchPair(pre, lr, wd)
        with torch.no_grad():               # this step's starting point is ours
            ref.p32.copy_(pre)
            ref.p64.copy_(pre.double())
        ref.step(grads * _clip_coef(norm, max_norm))
        ref.check(f"Trainer adam step {step + 1}", tr.flat.flat, tr.optimizer.exp_avg,
                  tr.optimizer.exp_avg_sq)
        assert int(tr.optimizer.step_count.item()) == step + 1
    pkg = dsm.DeepSpeech.serialize(tr.model, optimizer=tr.optimizer)
    assert 'betas' in pkg['optim_dict']['param_groups'][0]
    m2 = dsm.DeepSpeech.load_model_package(pkg)
    tr2 = Trainer(m2, LABELS, lr=0.5, max_norm=max_norm, device=dev, verbose=False,
                  optimizer='adam', weight_decay=1e-4, betas=(0.8, 0.99), eps=1e-6)
    o2 = tr2.optimizer
    assert (o2.lr, o2.betas, o2.eps, o2.weight_decay) == (0.5, (0.8, 0.99), 1e-6, 1e-4)
    tr2.optimizer.load_state_dict(pkg['optim_dict'])
    o1, o2 = tr.optimizer, tr2.optimizer
    assert int(o2.step_count.item()) == 2
    assert (o2.lr, o2.betas, o2.eps, o2.weight_decay) == (lr, BETAS, EPS, wd)
    assert torch.equal(o2.exp_avg, o1.exp_avg) and torch.equal(o2.exp_avg_sq, o1.exp_avg_sq)
    assert torch.equal(tr2.flat.flat, tr.flat.flat)
    assert o1.exp_avg.abs().max().item() > 0
