"""Shared by the BatchNorm tests (not a test module): the cases of tests/test_gpu_bn.py and their
references, built on the CPU.  Every input is drawn in float32 and a reference of dtype float64
(the reference) or float32 (one more draw of the float32 rounding error: the yardstick d32 of
w2l_common.bound) starts from those same bits.  References are computed once per case and
shared; nobody writes into them.

rows   : x [R, C], BatchNorm1d in training mode (F.batch_norm + autograd) and in eval mode.
planes : z0 [N, C, D, T] + b[c] with lens -- the chain of test_conv_block_fwd_bwd without the
         convolution: z = mask(z0 + b), BN(train), mask, hardtanh(0, 20), mask (model.py:63-79)
         -- and an unmasked variant (plain BatchNorm2d).
"""
import functools

import torch
import torch.nn.functional as F

from w2l_common import rel, bound  # noqa: F401  (re-exported: the tests take them from here)

EPS, MOMENTUM = 1e-5, 0.1
LO, HI = 0.0, 20.0

# ---------------------------------------------------------------------------- rows
# R: per = ceil(R / 256) rows per chunk of the rows reduction takes 1, 1, 2, 5, 8, 9, 13 (ragged or
# empty trailing chunks; from per = 5 on the float4 kernel's two-rows-in-flight loop runs).
# C: 4 / 64 / 260 take the float4 kernels (260: a second 256-column block one lane wide),
# 1 / 3 / 65 / 130 the scalar ones (one, two and three 64-column blocks).
ROWS_SHAPES = [(3, 4), (3, 1), (3, 65),
               (255, 64), (255, 3),
               (257, 260), (257, 130),
               (1279, 64), (1279, 65), (1279, 4), (1279, 1),
               (2048, 260), (2048, 130), (2048, 4),
               (2049, 64), (2049, 3), (2049, 65),
               (3300, 4), (3300, 130), (3300, 260), (3300, 3)]
OFFSET_SHAPES = [(2049, 12), (2049, 13)]
OFFSET_KINDS = ["off1000", "off100"]
UNALIGNED_SHAPE = (1279, 64)
EVAL_SHAPES = [(1279, 64), (57, 65)]
# (R, C, seed): seeds under which no pre-ReLU value lies within RELU_MARGIN of 0
# (test_bn_reference_cpu.py holds them to it)
BN_RELU_CASES = [(2049, 64, 4), (1279, 65, 1)]
RELU_MARGIN = 1e-5


def rows_inputs(r, c, seed=0, kind="std"):
    """float32 x [r, c], gamma, beta, dy and non-default running statistics.  kind: 'std'
    3 randn + 1, 'off1000' 1000 + 0.01 randn, 'off100' 100 + randn (means far from 0 against
    the spread: what an fp32 sum or an fp32-rounded mean loses)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * r + c)
    z = torch.randn(r, c, generator=g)
    x = {"std": lambda: z * 3 + 1, "off1000": lambda: 1000 + 0.01 * z,
         "off100": lambda: 100 + z}[kind]()
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    dy = torch.randn(r, c, generator=g)
    if kind != "std":
        # a gradient correlated with the input (any loss that grows with |y| gives one): the
        # xhat * mean(g xhat) term of dx then carries weight, and with it the mean inside xhat
        dy = dy + 2 * z
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, rm=torch.randn(c, generator=g),
                rv=torch.rand(c, generator=g) + 0.5)


def rows_reference(inp, dtype, relu=False):
    """F.batch_norm in training mode [+ ReLU] and its autograd gradients, in dtype."""
    x, gamma, beta = (inp[k].to(dtype).clone().requires_grad_(True)
                      for k in ("x", "gamma", "beta"))
    rm, rv = inp["rm"].to(dtype).clone(), inp["rv"].to(dtype).clone()
    pre = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=MOMENTUM, eps=EPS)
    y = F.relu(pre) if relu else pre
    y.backward(inp["dy"].to(dtype))
    return dict(y=y.detach(), pre=pre.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad,
                running_mean=rm, running_var=rv)


def rows_eval_reference(inp, dtype):
    """F.batch_norm in eval mode on the (non-trivial) running statistics of inp."""
    a = {k: v.to(dtype) for k, v in inp.items()}
    return F.batch_norm(a["x"], a["rm"], a["rv"], a["gamma"], a["beta"], training=False, eps=EPS)


@functools.lru_cache(maxsize=None)
def rows_case(r, c, seed=0, kind="std", relu=False):
    """(inputs, float64 reference, float32 reference) of one rows case."""
    inp = rows_inputs(r, c, seed, kind)
    return inp, rows_reference(inp, torch.float64, relu), rows_reference(inp, torch.float32, relu)


ROWS_TENSORS = ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")


def d32(case, name):
    """The yardstick: distance of the float32 CPU reference from the float64 one."""
    _, r64, r32 = case
    return rel(r32[name], r64[name])


# ---------------------------------------------------------------------------- planes
# (n, c, d, t, lens, seed).  The seeds keep every unmasked pre-clamp value at least CLAMP_MARGIN
# away from 0 and 20 (test_bn_reference_cpu.py holds them to it), so the GPU test compares the
# gradient with no exclusions.
PLANES_CASES = [
    # D = 5 straddles channels inside a 64-row f tile; an empty sample
    (3, 5, 5, 70, (70, 33, 0), 0),
    # the D == 1 split of T; a length beyond T; T one past the 256-thread stride
    (2, 3, 1, 257, (300, 1), 0),
    # D < kPlaneSplit; the odd-D tail of the two-chain backward; exact tile
    (4, 2, 3, 64, (64, 63, 1, 0), 2),
    # BA_ROWS remainder 1; T one past a tile; F = 63
    (2, 7, 9, 65, (65, 40), 0),
    # the model's channel count; the stats loop's 2 x 256 unroll plus tail (inner = 1200)
    (2, 32, 2, 600, (600, 257), 7),
    # smallest planes case
    (1, 1, 2, 1, (1,), 0),
    # D T = 1 with a mask
    (3, 4, 1, 1, (1, 0, 1), 0),
]
UNMASKED_CASES = [(3, 5, 5, 70, 0), (2, 3, 1, 257, 0)]
CLAMP_MARGIN = 2e-4      # ~20 x the fp32 rounding of a value <= 40 through the apply's four ops
CLAMP_SHARE = 0.05       # of the unmasked values on each clamp side ...
CLAMP_SHARE_FROM = 500   # ... in cases with more unmasked values than this


def planes_id(case):
    n, c, d, t = case[:4]
    return f"{n}x{c}x{d}x{t}"


def time_mask(lens, t):
    """[n, 1, 1, t] bool, True at the padded positions t >= lens[n]."""
    m = torch.arange(t)[None, :] >= torch.as_tensor(lens)[:, None].long()
    return m[:, None, None, :]


def planes_inputs(n, c, d, t, lens, seed=0):
    """float32 z0, b, gamma ~ U(4, 8), beta ~ N(10, 3), dy in both layouts, running statistics,
    and z = mask(z0 + b[c]) in float32: the bits the HIP kernels and the references start from."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * n + 17 * c + 5 * d + t)
    z0 = torch.randn(n, c, d, t, generator=g) * 2 + 0.5
    b = torch.randn(c, generator=g)
    inp = dict(z0=z0, b=b, gamma=torch.rand(c, generator=g) * 4 + 4,
               beta=torch.randn(c, generator=g) * 3 + 10,
               dy0=torch.randn(n, c, d, t, generator=g),
               dy1=torch.randn(t, n, c * d, generator=g), rm=torch.randn(c, generator=g),
               rv=torch.rand(c, generator=g) + 0.5,
               lens=torch.tensor(lens, dtype=torch.int32))
    zb = z0 + b[None, :, None, None]
    inp["zb"] = zb                                            # unmasked: the plain-BN variant's x
    inp["z"] = zb.masked_fill(time_mask(lens, t), 0)
    return inp


def to_layout1(y):
    """[n, c, d, t] -> the [t, n, c d] collapse of model.py:360-362."""
    n, c, d, t = y.shape
    return y.reshape(n, c * d, t).permute(2, 0, 1)


def planes_reference(inp, dtype, layout):
    """mask -> BN(train) -> mask -> hardtanh -> mask on the float32 sum's bits, dy in `layout`.
    b enters through a term that is exactly zero, so z keeps those bits and autograd still
    returns b's gradient (the closed-form dbias of the backward's final kernel)."""
    lens = inp["lens"]
    n, c, d, t = inp["z0"].shape
    m = time_mask(lens, t)
    b = inp["b"].to(dtype).clone().requires_grad_(True)
    gamma = inp["gamma"].to(dtype).clone().requires_grad_(True)
    beta = inp["beta"].to(dtype).clone().requires_grad_(True)
    rm, rv = inp["rm"].to(dtype).clone(), inp["rv"].to(dtype).clone()
    zsum = inp["zb"].to(dtype).clone().requires_grad_(True)
    z = (zsum + (b - b.detach())[None, :, None, None]).masked_fill(m, 0)
    pre = F.batch_norm(z, rm, rv, gamma, beta, training=True, momentum=MOMENTUM,
                       eps=EPS).masked_fill(m, 0)
    y = F.hardtanh(pre, LO, HI).masked_fill(m, 0)
    out = y if layout == 0 else to_layout1(y)
    out.backward(inp["dy0" if layout == 0 else "dy1"].to(dtype))
    return dict(y=y.detach(), pre=pre.detach(), unmasked=~m.expand(n, c, d, t), dz=zsum.grad,
                dgamma=gamma.grad, dbeta=beta.grad, db=b.grad, running_mean=rm, running_var=rv)


def planes_plain_reference(inp, dtype):
    """The unmasked variant: plain BatchNorm2d (training) on zb with dy0, no lens, no clamp."""
    x, gamma, beta = (inp[k].to(dtype).clone().requires_grad_(True)
                      for k in ("zb", "gamma", "beta"))
    rm, rv = inp["rm"].to(dtype).clone(), inp["rv"].to(dtype).clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=MOMENTUM, eps=EPS)
    y.backward(inp["dy0"].to(dtype))
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm,
                running_var=rv)


@functools.lru_cache(maxsize=None)
def planes_case(n, c, d, t, lens, seed=0):
    """(inputs, {layout: float64 reference}, {layout: float32 reference})."""
    inp = planes_inputs(n, c, d, t, lens, seed)
    return (inp, {l: planes_reference(inp, torch.float64, l) for l in (0, 1)},
            {l: planes_reference(inp, torch.float32, l) for l in (0, 1)})


@functools.lru_cache(maxsize=None)
def planes_plain_case(n, c, d, t, seed=0):
    inp = planes_inputs(n, c, d, t, (t,) * n, seed)
    return (inp, planes_plain_reference(inp, torch.float64),
            planes_plain_reference(inp, torch.float32))


PLANES_TENSORS = ("dz", "dgamma", "dbeta", "db")
