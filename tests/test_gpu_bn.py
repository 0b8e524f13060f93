"""GPU: the BatchNorm kernels of csrc/bn.hip against float64 at their reduction, mask and layout
edges (the cases and references of bn_common; no convolution in front, so shapes are free).

Bounds are this project's existing ones: y, dgamma, dbeta and the running statistics 1e-5, dx
1e-4 (test_seq_bn_fwd_bwd); BatchNorm + ReLU 1e-5 throughout (test_bn_relu_fwd_bwd); the masked
BatchNorm2d gradients 2e-4 (test_conv_block_fwd_bwd); all relative to the tensor's largest
reference magnitude (w2l_common.rel).  Each comparison prints the HIP error next to d32, the
float32 CPU reference's distance from float64 (pytest -s; profiles/bn_parity.txt is that output).
"""
import pytest
import torch

from ds2amd import ops, _lib
import bn_common as bc

pytestmark = pytest.mark.gpu

INVALID_VALUE, UNSUPPORTED_SHAPE, WORKSPACE_TOO_SMALL = 1, 2, 5
ROWS_BOUNDS = dict(y=1e-5, dx=1e-4, dgamma=1e-5, dbeta=1e-5, running_mean=1e-5, running_var=1e-5)
BN_RELU_BOUNDS = dict.fromkeys(bc.ROWS_TENSORS, 1e-5)
PLANES_BOUND = 2e-4


class _Report:
    """Prints every comparison of a test first and fails at the end, so one miss does not hide
    the other tensors' figures."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def close(self, name, got, ref, limit, d32=None):
        err = bc.rel(got, ref)
        d = "-" if d32 is None else f"{d32:.3e}"
        print(f"{self.tag} {name}: d32 {d} ours {err:.3e} bound {limit:.3e}")
        if not err <= limit:
            self.bad.append(f"{name}: {err:.3e} > {limit:.3e}")

    def true(self, name, cond):
        if not cond:
            self.bad.append(name)

    def done(self):
        assert not self.bad, f"{self.tag}: " + "; ".join(self.bad)


def _seq_bn(dev, inp, fn=ops.SeqBatchNormFn, x_dev=None):
    """Training forward + backward of SeqBatchNormFn / BNReLUFn on the case's float32 inputs."""
    xd = (inp["x"].to(dev) if x_dev is None else x_dev).requires_grad_(True)
    gd = inp["gamma"].to(dev).requires_grad_(True)
    bd = inp["beta"].to(dev).requires_grad_(True)
    rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
    y = fn.apply(xd, gd, bd, rm, rv, True, bc.MOMENTUM, bc.EPS)
    y.backward(inp["dy"].to(dev))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad, running_mean=rm,
                running_var=rv)


def _compare_rows(rep, case, out, bounds):
    _, r64, _ = case
    for k in bc.ROWS_TENSORS:
        rep.close(k, out[k], r64[k], bounds[k], bc.d32(case, k))
        rep.true(f"{k} finite", torch.isfinite(out[k]).all().item())


def _bit_identical(rep, a, b):
    for k in a:
        rep.true(f"{k} differs between two runs", torch.equal(a[k], b[k]))


# ---------------------------------------------------------------------------- a. rows reduction
@pytest.mark.parametrize("r,c", bc.ROWS_SHAPES)
def test_seq_bn_rows_vs_fp64(dev, r, c):
    """SeqBatchNormFn train forward + backward where per = ceil(R / 256) rows per chunk is 1, 2,
    5, 8, 9 and 13 (one row per group; ragged and empty chunks; the float4 kernel's paired loop
    with and without its one-row tail) on the float4 (C % 4 == 0) and the scalar kernels, from
    non-default running statistics; two runs bit-identical (fixed-order sums)."""
    case = bc.rows_case(r, c)
    rep = _Report(f"rows {r}x{c}")
    out = _seq_bn(dev, case[0])
    _compare_rows(rep, case, out, ROWS_BOUNDS)
    _bit_identical(rep, out, _seq_bn(dev, case[0]))
    rep.done()


# ---------------------------------------------------------------------------- b. one row
@pytest.mark.parametrize("c", [64, 65])
def test_seq_bn_single_row(dev, c):
    """R = 1 (torch refuses it in training): the batch mean is the row, the variance 0, so
    y == beta exactly, dx == 0, dgamma == 0, dbeta == dy; the running mean moves towards x and
    the running variance by momentum * 0 (the count > 1 guard: no 0 / 0); everything finite.
    dx is exact because the backward's final kernel takes k1 = 0 for a count of 1 (the apply's
    fused k1 g - k1 mean(g) alone leaves a rounding)."""
    inp = bc.rows_inputs(1, c)
    out = _seq_bn(dev, inp)
    rep = _Report(f"rows 1x{c}")
    for k, v in out.items():
        rep.true(f"{k} finite", torch.isfinite(v).all().item())
    print(f"rows 1x{c}: max |dx| {out['dx'].abs().max().item():.1e}, max |dgamma| "
          f"{out['dgamma'].abs().max().item():.1e}")
    rep.true("y == beta", torch.equal(out["y"].cpu(), inp["beta"][None, :]))
    rep.true("dx == 0", not out["dx"].any().item())
    rep.true("dgamma == 0", not out["dgamma"].any().item())
    rep.true("dbeta == dy", torch.equal(out["dbeta"].cpu(), inp["dy"][0]))
    m = bc.MOMENTUM
    rep.close("running_mean", out["running_mean"],
              (1 - m) * inp["rm"].double() + m * inp["x"][0].double(), 1e-5)
    rep.close("running_var", out["running_var"], (1 - m) * inp["rv"].double(), 1e-5)
    rep.done()


# ---------------------------------------------------------------------------- c. offset mean
@pytest.mark.parametrize("r,c", bc.OFFSET_SHAPES)
@pytest.mark.parametrize("kind", bc.OFFSET_KINDS)
def test_seq_bn_offset_mean(dev, kind, r, c):
    """The header's two numerical claims as assertions.  x = 1000 + 0.01 randn with a gradient
    correlated with x: y within bound(d32) of float64 (the forward keeps the fp32-rounded mean,
    as torch's float32 does: d32 6e-4 .. 3e-3 by host, HIP 3.3e-4 / 6.6e-4), while dx stays
    within 1e-4 and dgamma within 1e-5 (measured 1.4e-6 .. 1.8e-6 and 7e-7 .. 9e-7; the float32
    CPU reference: 1.4e-3 .. 5.7e-3 and 2e-4 .. 6e-4) because the sums run in fp64 and the
    backward takes the batch mean exactly.  float accumulators in the float4 reduction put y
    and dgamma of the C = 12 cases outside; the fp32 mean in the backward apply puts dx at
    7e-4 .. 1e-3.  x = 100 + randn: every standard bound."""
    case = bc.rows_case(r, c, 0, kind)
    rep = _Report(f"rows {kind} {r}x{c}")
    out = _seq_bn(dev, case[0])
    bounds = dict(ROWS_BOUNDS)
    if kind == "off1000":
        bounds["y"] = bc.bound(bc.d32(case, "y"))
    _compare_rows(rep, case, out, bounds)
    rep.done()


# ---------------------------------------------------------------------------- d. unaligned
def test_seq_bn_unaligned_operand(dev, monkeypatch):
    """x at a 4-byte offset from a 16-byte boundary (contiguous, C % 4 == 0): the float4
    reductions, the float4 apply and ds2_bn_apply_amax all give way to the scalar kernels.  Same
    bounds; no row / column maxima are left for the output (bn_apply_amax's documented
    fallback)."""
    monkeypatch.setenv("DS2_GEMM_H3", "1")
    monkeypatch.setenv("DS2_GEMM_X6", "1")
    r, c = bc.UNALIGNED_SHAPE
    case = bc.rows_case(r, c)
    inp = case[0]
    rep = _Report(f"rows unaligned {r}x{c}")

    def unaligned_x():
        buf = torch.zeros(r * c + 8, device=dev)
        x = buf[1:1 + r * c].view(r, c)
        x.copy_(inp["x"])
        assert x.is_contiguous() and x.data_ptr() % 16 == 4
        return x
    out = _seq_bn(dev, inp, x_dev=unaligned_x())
    _compare_rows(rep, case, out, ROWS_BOUNDS)
    _bit_identical(rep, out, _seq_bn(dev, inp, x_dev=unaligned_x()))
    rep.true("no maxima for the unaligned operand's output",
             ops._take_amax(out["y"], r, c) == (None, None))
    # the aligned operand does leave them (what the fallback gives up)
    aligned = _seq_bn(dev, inp)
    rep.true("maxima for the aligned operand's output",
             ops._take_amax(aligned["y"], r, c)[0] is not None)
    # bn_apply_amax itself: the fallback's y equals the aligned call's
    x_u = unaligned_x()
    mean, invstd = ops.bn_stats(x_u, r, c, 1, bc.EPS, bc.MOMENTUM, None, None, True)
    gd, bd = inp["gamma"].to(dev), inp["beta"].to(dev)
    y_u = ops.bn_apply_amax(x_u, r, c, mean, invstd, gd, bd)
    y_a = ops.bn_apply_amax(inp["x"].to(dev), r, c, mean, invstd, gd, bd)
    rep.true("fallback y == bn_apply_amax y", torch.equal(y_u, y_a))
    rep.true("fallback leaves no maxima", ops._take_amax(y_u, r, c) == (None, None))
    ops._take_amax(y_a, r, c)
    rep.done()


# ---------------------------------------------------------------------------- e. eval mode
@pytest.mark.parametrize("r,c", bc.EVAL_SHAPES)
def test_seq_bn_eval(dev, r, c):
    """training=False (ds2_bn_eval_stats): y from the running statistics vs float64 eval
    F.batch_norm; the running statistics unchanged bit for bit; backward raises."""
    inp = bc.rows_inputs(r, c)
    rep = _Report(f"rows eval {r}x{c}")
    xd = inp["x"].to(dev).requires_grad_(True)
    rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
    y = ops.SeqBatchNormFn.apply(xd, inp["gamma"].to(dev), inp["beta"].to(dev), rm, rv, False,
                                 bc.MOMENTUM, bc.EPS)
    rep.close("y", y, bc.rows_eval_reference(inp, torch.float64), 1e-5,
              bc.rel(bc.rows_eval_reference(inp, torch.float32),
                     bc.rows_eval_reference(inp, torch.float64)))
    rep.true("running_mean unchanged", torch.equal(rm.cpu(), inp["rm"]))
    rep.true("running_var unchanged", torch.equal(rv.cpu(), inp["rv"]))
    with pytest.raises(_lib.Ds2Error):
        y.backward(inp["dy"].to(dev))
    rep.done()


# ---------------------------------------------------------------------------- f. BN + ReLU
@pytest.mark.parametrize("r,c,seed", bc.BN_RELU_CASES)
def test_bn_relu_rows_vs_fp64(dev, r, c, seed):
    """BNReLUFn (ds2_bn_backward under ds2_bn_relu_bwd) where the reduction's paired loop runs:
    (2049, 64) float4 with tail, (1279, 65) scalar; test_bn_relu_fwd_bwd's bounds."""
    case = bc.rows_case(r, c, seed, "std", True)
    rep = _Report(f"bn_relu {r}x{c}")
    out = _seq_bn(dev, case[0], fn=ops.BNReLUFn)
    _compare_rows(rep, case, out, BN_RELU_BOUNDS)
    rep.true("ReLU pattern", torch.equal(out["y"].cpu() > 0, case[1]["y"] > 0))
    rep.done()


# ---------------------------------------------------------------------------- g. planes, masked
def _apply_mask_htanh(z, n, c, d, t, mean, invstd, gamma, beta, lens, layout):
    """ds2_bn_apply_mask_htanh as ConvBlockFn.forward calls it."""
    y = (torch.full((t, n, c * d), float("nan"), device=z.device) if layout == 1
         else torch.full_like(z, float("nan")))
    _lib.call("ds2_bn_apply_mask_htanh", z.data_ptr(), n, c, d, t, mean.data_ptr(),
              invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ops._p(lens), float(bc.LO),
              float(bc.HI), y.data_ptr(), int(layout), ops._stream())
    return y


def _to_ncdt(dy1, n, c, d, t):
    return dy1.permute(1, 2, 0).reshape(n, c, d, t)


@pytest.mark.parametrize("case", bc.PLANES_CASES, ids=bc.planes_id)
def test_planes_masked_vs_fp64(dev, case):
    """ds2_bn_train_stats (inner = D T) -> ds2_bn_apply_mask_htanh in both layouts ->
    ds2_bn_backward(masked, dbias) with dy in both layouts, against mask -> BN -> mask ->
    hardtanh(0, 20) -> mask in float64.  y 1e-5 in both layouts, the [T, N, C D] output the
    permuted [N, C, D, T] one bit for bit, masked positions exactly 0 in y and dz, the Hardtanh's
    pass / block pattern the reference's at every element (bn_common keeps every value 2e-4 from
    the bounds), dz / dgamma / dbeta / dbias 2e-4, running statistics 1e-5.

    Where no position is masked the bias gradient is analytically 0 (a BatchNorm's dx sums to 0
    per channel) and the reference holds rounding noise: HIP must return exactly 0 there.

    1x1x2x1: with two values per channel dz = +-k1 (g1 - g2) / 2 * (1 - xhat^2) and
    1 - xhat^2 = eps * invstd^2 ~ 3e-6, so the fp32 rounding of the stored invstd (<= 6e-8) is
    up to percents of it (4.4e-3 measured; the float32 CPU reference 9.0e-3 / 2.0e-2).  Given
    the forward's eps, the backward takes the invstd of channels of at most 8 values from x in
    fp64 and meets the bound."""
    n, c, d, t, lens_t, _ = case
    inp, r64, r32 = bc.planes_case(*case)
    tag = f"planes {bc.planes_id(case)}"
    rep = _Report(tag)
    z, lens = inp["z"].to(dev), inp["lens"].to(dev)
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
    mean, invstd = ops.bn_stats(z, n, c, d * t, bc.EPS, bc.MOMENTUM, rm, rv, True)
    ref = r64[0]
    unmasked = ref["unmasked"]
    rep.close("running_mean", rm, ref["running_mean"], 1e-5, bc.rel(r32[0]["running_mean"],
                                                                    ref["running_mean"]))
    rep.close("running_var", rv, ref["running_var"], 1e-5, bc.rel(r32[0]["running_var"],
                                                                  ref["running_var"]))
    y0 = _apply_mask_htanh(z, n, c, d, t, mean, invstd, gamma, beta, lens, 0).cpu()
    y1 = _apply_mask_htanh(z, n, c, d, t, mean, invstd, gamma, beta, lens, 1).cpu()
    d32y = bc.rel(r32[0]["y"], ref["y"])
    rep.close("y layout 0", y0, ref["y"], 1e-5, d32y)
    rep.close("y layout 1", y1, bc.to_layout1(ref["y"]), 1e-5, d32y)
    rep.true("y layout 1 == permuted layout 0", torch.equal(y1, bc.to_layout1(y0)))
    rep.true("y == 0 at masked positions", not y0[~unmasked].any().item())
    passed = (ref["pre"] > bc.LO) & (ref["pre"] < bc.HI) & unmasked
    rep.true("forward clamp pattern", torch.equal((y0 > bc.LO) & (y0 < bc.HI), passed))
    none_masked = bool(unmasked.all())
    k1 = (inp["gamma"].double() / (inp["z"].double().var((0, 2, 3), unbiased=False)
                                   + bc.EPS).sqrt())[None, :, None, None]
    for layout in (0, 1):
        ref = r64[layout]
        dy = inp["dy0" if layout == 0 else "dy1"]
        dz, dgamma, dbeta, db = ops.bn_backward(dy.to(dev), layout, z, n, c, d, t, mean, invstd,
                                                gamma, beta, masked=True, lens=lens, lo=bc.LO,
                                                hi=bc.HI, want_dbias=True, eps=bc.EPS)
        dz = dz.cpu()
        for k, v in (("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta)):
            rep.close(f"{k} (dy layout {layout})", v, ref[k], PLANES_BOUND,
                      bc.rel(r32[layout][k], ref[k]))
        if none_masked:
            noise = ref["db"].abs().max().item() / ref["dz"].abs().sum().item()
            print(f"{tag} db (dy layout {layout}): analytically 0, reference noise {noise:.1e} "
                  f"of sum |dz|, ours {db.abs().max().item():.1e}")
            rep.true("reference db is rounding noise", noise < 1e-12)
            rep.true(f"db == 0 (dy layout {layout})", not db.any().item())
        else:
            rep.close(f"db (dy layout {layout})", db, ref["db"], PLANES_BOUND,
                      bc.rel(r32[layout]["db"], ref["db"]))
        rep.true(f"dz == 0 at masked positions (dy layout {layout})",
                 not dz[~unmasked].any().item())
        # the backward's pass / block decisions: one flipped element moves its dz by
        # k1 |dy|; nowhere may HIP be half of that (plus the fp32 resolution of dz) from the
        # reference
        dyn = (dy if layout == 0 else _to_ncdt(dy, n, c, d, t)).double()
        flip = (k1 * dyn.abs()).masked_fill(~unmasked, float("inf"))
        res = 1e-5 * ref["dz"].abs().max().item()
        rep.true(f"backward clamp pattern (dy layout {layout})",
                 ((dz.double() - ref["dz"]).abs() < 0.5 * flip + res).all().item())
    rep.done()


# ---------------------------------------------------------------------------- h. planes, unmasked
@pytest.mark.parametrize("n,c,d,t,seed", bc.UNMASKED_CASES)
def test_planes_unmasked_vs_fp64(dev, n, c, d, t, seed):
    """Plain BatchNorm2d over [N, C, D T]: the planes statistics, ds2_bn_apply with inner > 1
    (the generic apply kernel) and ds2_bn_backward(masked=0) with d t > 1, vs float64."""
    inp, r64, r32 = bc.planes_plain_case(n, c, d, t, seed)
    rep = _Report(f"planes unmasked {n}x{c}x{d}x{t}")
    x = inp["zb"].to(dev)
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
    mean, invstd = ops.bn_stats(x, n, c, d * t, bc.EPS, bc.MOMENTUM, rm, rv, True)
    y = ops.bn_apply(x, n, c, d * t, mean, invstd, gamma, beta)
    dx, dgamma, dbeta, _ = ops.bn_backward(inp["dy0"].to(dev), 0, x, n, c, d, t, mean, invstd,
                                           gamma, beta, masked=False, eps=bc.EPS)
    out = dict(y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv)
    for k in bc.ROWS_TENSORS:
        rep.close(k, out[k], r64[k], ROWS_BOUNDS[k], bc.rel(r32[k], r64[k]))
    rep.done()


# ---------------------------------------------------------------------------- i. argument checks
def test_bn_argument_checks(dev):
    """Statuses of the entry points' own checks (each returns before any launch)."""
    lib = _lib.load()
    n, c, d, t = 2, 4, 3, 5
    x = torch.randn(n, c, d, t, device=dev)
    dy, dx = torch.randn_like(x), torch.empty_like(x)
    v = [torch.ones(c, device=dev) for _ in range(7)]
    mean, invstd, gamma, beta, dgamma, dbeta, _ = v
    lens = torch.tensor([t, 2], dtype=torch.int32, device=dev)
    nbytes = _lib.size("ds2_bn_workspace_size", n, c, d * t)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def backward(layout, masked, lens_ptr, ws_bytes):
        return lib.ds2_bn_backward(dy.data_ptr(), layout, x.data_ptr(), n, c, d, t,
                                   mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                   beta.data_ptr(), masked, lens_ptr, 0.0, 20.0, 1e-5,
                                   dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), None,
                                   ws.data_ptr(), ws_bytes, ops._stream())
    assert backward(1, 0, None, nbytes) == INVALID_VALUE
    assert backward(0, 1, None, nbytes) == INVALID_VALUE
    assert backward(0, 0, None, nbytes - 1) == WORKSPACE_TOO_SMALL
    assert backward(0, 1, lens.data_ptr(), nbytes - 1) == WORKSPACE_TOO_SMALL
    assert backward(0, 1, lens.data_ptr(), nbytes) == 0
    # D T = 1 with a mask is sized by the same query
    nb1 = _lib.size("ds2_bn_workspace_size", n, c, 1)
    assert lib.ds2_bn_backward(dy.data_ptr(), 0, x.data_ptr(), n, c, 1, 1, mean.data_ptr(),
                               invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1,
                               lens.data_ptr(), 0.0, 20.0, 1e-5, dx.data_ptr(), dgamma.data_ptr(),
                               dbeta.data_ptr(), None, ws.data_ptr(), nb1 - 1,
                               ops._stream()) == WORKSPACE_TOO_SMALL
    assert lib.ds2_bn_train_stats(x.data_ptr(), n, c, d * t, 1e-5, 0.1, mean.data_ptr(),
                                  invstd.data_ptr(), None, None, ws.data_ptr(), nbytes - 1,
                                  ops._stream()) == WORKSPACE_TOO_SMALL
    rows, wide = 2, 2052
    xw = torch.zeros(rows, wide, device=dev)
    p = [torch.ones(wide, device=dev) for _ in range(4)]
    rmax = torch.empty(rows, dtype=torch.int32, device=dev)
    cmax = torch.empty(wide, dtype=torch.int32, device=dev)
    assert lib.ds2_bn_apply_amax(xw.data_ptr(), rows, wide, *[q.data_ptr() for q in p],
                                 torch.empty_like(xw).data_ptr(), rmax.data_ptr(),
                                 cmax.data_ptr(), ops._stream()) == UNSUPPORTED_SHAPE
    torch.cuda.synchronize()
