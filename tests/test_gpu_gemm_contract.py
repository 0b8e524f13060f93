"""GPU: the GEMM family against float64 across its calling contract -- padded leading
dimensions and offsets inside poisoned allocations, beta = 0 over NaN, strided batches, the
workspace ladder -- with every case first asserting the rung and split the library's own plan
(ds2_test_sgemm_plan) gives for exactly that call.

The entry points are called directly (tests/gemm_common.py run_gemm): ops.sgemm cannot express
batches, strides or a short workspace.  alpha = 0.5, beta = 0.25 and a bias unless a case says
otherwise, so a piece covered twice or an epilogue applied twice shows.  All poison lies inside
live allocations that span every rows x ld extent a kernel may address.
"""
import numpy as np
import pytest
import torch

from ds2amd import _lib, ops

from gemm_common import (SHAPES, TRANS, CANARY, WS_FULL, WS_NONE, WS_SLABS, WS_SLABS_LESS_1, Slab,
                         operand, ref64, close, run_gemm, gemm_env, rows16, H3_CASES, h3_case,
                         h3_maxima, h3_bound, normal_range, bits_of)

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (name, kind, mode, shape): every rung the shapes reach
RUNG_CASES = [
    ("h3_160", "sgemm", "h3", "S"), ("h3_128", "sgemm", "h3", "S-narrow"),
    ("x6_m16_160", "sgemm", "x6", "S"), ("x6_m16_128", "sgemm", "x6", "S-narrow"),
    ("x6_k_160", "sgemm", "h3", "S-ktail"), ("x6_k_128", "sgemm", "h3", "S-ktail-narrow"),
    ("f64_128", "sgemm", "fp32", "S"), ("f64_128-narrow", "sgemm", "fp32", "S-narrow"),
    ("f64_128-ktail", "sgemm", "fp32", "S-ktail"),
    ("f16", "sgemm", "h3", "S-odd"), ("f16-fp32", "sgemm", "fp32", "S-odd"),
    ("bf16_staged", "sgemm_bf16", "h3", "S"), ("bf16_staged-ktail", "sgemm_bf16", "h3", "S-ktail"),
    ("bf16_dma", "bgemm_nt", "h3", "S"), ("bf16_dma_k", "bgemm_nt", "h3", "S-ktail8"),
]
RUNG_IDS = [c[0] for c in RUNG_CASES]


def expected_rung(kind, mode, m, n, k, batch=1):
    """DESIGN.md's GEMM dispatch table for operands staged as float4 wherever m, n, k allow."""
    if kind == "sgemm_bf16":
        return "bf16_staged"
    if kind == "bgemm_nt":
        return "bf16_dma_k" if k % 64 else "bf16_dma"
    if m % 4 or n % 4 or k % 4:
        return "f16"
    if mode == "fp32":
        return "f64_128"                       # (the plan's time model takes 128 at these sizes)
    wide = "160" if n >= 256 else "128"
    if k % 32:
        return "x6_k_" + wide
    return ("h3_" if mode == "h3" and batch == 1 else "x6_m16_") + wide


def trans_of(kind):
    return [(0, 1)] if kind == "bgemm_nt" else TRANS


def make_inputs(kind, m, n, k, ta, tb, seed, batch=1):
    """Stored operands (A [m][k] or [k][m], B [k][n] or [n][k]), C0 and bias on the CPU; the
    bf16 kinds get bf16-representable values, so the float64 product of the same values is
    their reference too (ds2_sgemm_bf16_ws rounds on the way in: a no-op on them)."""
    g = torch.Generator().manual_seed(seed)
    a = [torch.randn((k, m) if ta else (m, k), generator=g) for _ in range(batch)]
    b = [torch.randn((n, k) if tb else (k, n), generator=g) for _ in range(batch)]
    c0 = [torch.randn(m, n, generator=g) for _ in range(batch)]
    bias = torch.randn(n, generator=g)
    if kind != "sgemm":
        a = [x.to(torch.bfloat16) for x in a]
        b = [x.to(torch.bfloat16) for x in b]
        if kind == "sgemm_bf16":
            a, b = [x.float() for x in a], [x.float() for x in b]
    return a, b, c0, bias


def check(C, refs, plan, name):
    got = C.read()
    for i, (g, r) in enumerate(zip(got, refs)):
        assert torch.isfinite(g).all().item(), f"{name}[{i}]: non-finite output ({plan})"
        close(g, r, 1e-5, f"{name}[{i}] {plan.rung} nsplit {plan.nsplit}")
    assert C.outside_unchanged(), f"{name}: a word outside C was written ({plan})"


# ------------------------------------------------------------------ a. padding and poison
@pytest.mark.parametrize("layout", ["ldc+4", "ldc+3", "model"])
@pytest.mark.parametrize("case", RUNG_CASES, ids=RUNG_IDS)
def test_padded_offset_operands_in_poison(dev, case, layout, monkeypatch):
    """lda = extent + 8, ldb = extent + 12, ldc = n + 4 (row-vector epilogue) or n + 3 (scalar),
    each operand at a nonzero 16-byte-aligned offset of a larger allocation whose every other
    element is NaN (A, B) or a canary word (C).  "model": the step's own forms -- C the columns
    [n, 2n) of an [m][2n] buffer, A the columns [m, 2m) of a [k][2m] buffer with trans_a, B a
    [k][2n] buffer's right half.  The result matches float64 at 1e-5 max |ref| and is finite
    (so no poison was read, the fp16x3 scale pre-pass included) and every canary is intact."""
    name, kind, mode, shape = case
    gemm_env(monkeypatch, mode)
    m, n, k = SHAPES[shape]
    wide = layout == "model"
    odd = shape == "S-odd"
    tr = [(0, 1)] if kind == "bgemm_nt" else [(1, 0)] if wide else TRANS
    gran = 8 if kind == "bgemm_nt" else 4        # elements per 16 bytes
    for ta, tb in tr:
        a, b, c0, bias = make_inputs(kind, m, n, k, ta, tb, 1000 * ta + 100 * tb + k + n)
        A = operand(a, ta, 8, gran, None, dev, wide=wide)
        B = operand(b, tb, 8 if kind == "bgemm_nt" else 12, 2 * gran, None, dev,
                    wide=wide and kind != "bgemm_nt")
        ldc = 2 * n if wide else n + (3 if layout == "ldc+3" else 4)
        C = Slab(c0, ldc, n if wide else 12, 0, CANARY, dev)
        biasd = bias.to(dev)
        plan = run_gemm(kind, dev, m=m, n=n, k=k, ta=ta, tb=tb, alpha=0.5, beta=0.25, A=A, B=B,
                        C=C, bias=biasd)
        assert plan.rung == expected_rung(kind, mode, m, n, k), (name, ta, tb, plan)
        assert plan.nsplit > 1, plan            # k / 256 = 4: the split and its reduce run
        if kind == "sgemm":
            assert plan.vec == rows16(C), plan
            assert odd or plan.vec == int(layout != "ldc+3"), plan
        refs = ref64(a, b, c0, bias, 0.5, 0.25, ta, tb)
        check(C, refs, plan, f"{name} {layout} ta{ta} tb{tb}")


# ------------------------------------------------------------------ b. beta == 0
UNSPLIT_K = {1024: 224, 1028: 228, 1021: 221, 1032: 232}


@pytest.mark.parametrize("variant", ["beta0", "beta0-scalar", "alpha0-beta1", "nobias"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "unsplit"])
@pytest.mark.parametrize("case", RUNG_CASES, ids=RUNG_IDS)
def test_beta_zero_does_not_read_c(dev, case, split, variant, monkeypatch):
    """beta == 0 over a C prefilled with NaN gives a finite, correct result: in the kernels'
    own epilogues (unsplit: K < 256, or no workspace for the bf16 kernels) and in both forms
    of the split reduce (16-byte: ldc = n + 4; scalar: "beta0-scalar", ldc = n + 3).  Also
    alpha = 0 with beta = 1 (C + bias exactly) and no bias, all four transposes for beta0,
    (0, 1) for the rest."""
    name, kind, mode, shape = case
    gemm_env(monkeypatch, mode)
    m, n, k = SHAPES[shape]
    ws = WS_FULL
    if not split:
        if kind == "sgemm":
            k = UNSPLIT_K[k]
        else:
            ws = WS_NONE
    alpha, beta = (0.0, 1.0) if variant == "alpha0-beta1" else (0.5, 0.0)
    if variant == "nobias":
        beta = 0.25
    gran = 8 if kind == "bgemm_nt" else 4
    for ta, tb in (trans_of(kind) if variant == "beta0" else [(0, 1)]):
        a, b, c0, bias = make_inputs(kind, m, n, k, ta, tb, 7 + 1000 * ta + 100 * tb + k + n)
        if beta == 0.0:
            c0 = [torch.full_like(c0[0], NAN)]
        A = operand(a, ta, 8, gran, None, dev)
        B = operand(b, tb, 8 if kind == "bgemm_nt" else 12, 2 * gran, None, dev)
        C = Slab(c0, n + (3 if variant == "beta0-scalar" else 4), 12, 0, CANARY, dev)
        biasd = None if variant == "nobias" else bias.to(dev)
        plan = run_gemm(kind, dev, m=m, n=n, k=k, ta=ta, tb=tb, alpha=alpha, beta=beta, A=A, B=B,
                        C=C, bias=biasd, ws=ws)
        if kind == "sgemm" or ws == WS_FULL:
            assert plan.rung == expected_rung(kind, mode, m, n, k), (name, plan)
        assert (plan.nsplit > 1) == split, plan
        refs = ref64(a, b, c0, None if biasd is None else bias, alpha, beta, ta, tb)
        check(C, refs, plan, f"{name} {variant} ta{ta} tb{tb}")
        if variant == "alpha0-beta1":      # nothing of the product may leak in: exact
            assert torch.equal(C.read()[0], c0[0] + bias), (name, plan)


# ------------------------------------------------------------------ c. strided batch
STRIDES = ["tight", "padded", "shared-b", "c+4", "c+1"]


@pytest.mark.parametrize("strides", STRIDES)
@pytest.mark.parametrize("shape", ["S", "S-narrow", "S-ktail", "S-odd"])
@pytest.mark.parametrize("kind,mode", [("sgemm", "h3"), ("sgemm", "fp32"), ("sgemm_bf16", "h3")],
                         ids=["sgemm", "sgemm-fp32", "sgemm_bf16"])
def test_strided_batch(dev, kind, mode, shape, strides, monkeypatch):
    """batch = 3: tight strides, padded ones (m * lda + 8), one B shared by the batch
    (stride_b = 0), stride_c = m * ldc + 4, and stride_c = m * ldc + 1, where entry 1 of C
    starts off 16-byte alignment and the split reduce must take its scalar form.  Never
    fp16x3; a per-entry float64 product at 1e-5; the gaps between the entries of C are
    canaries.  The staged-bf16 entry point rejects S-odd (no float4 staging) on the host."""
    gemm_env(monkeypatch, mode)
    m, n, k = SHAPES[shape]
    batch = 3
    odd = shape == "S-odd"
    if kind == "sgemm_bf16" and odd:
        a = torch.zeros(8, device=dev)
        st = _lib.load().ds2_sgemm_bf16_ws(0, 0, m, n, k, 1.0, a.data_ptr(), k, 0, a.data_ptr(),
                                           n, 0, 0.0, a.data_ptr(), n, 0, batch, None, None, 0,
                                           None)
        assert st == _lib.UNSUPPORTED_SHAPE
        return
    for ta, tb in TRANS:
        a, b, c0, bias = make_inputs(kind, m, n, k, ta, tb, 31 + 1000 * ta + 100 * tb + k + n,
                                     batch)
        pad = 8 if strides == "padded" else 0
        A = operand(a, ta, 8, 4, pad, dev)
        B = operand(b, tb, 12, 8, None if strides == "shared-b" else pad, dev)
        ldc = n + 4
        cpad = {"c+4": 4, "c+1": 1, "padded": 8}.get(strides, 0)
        C = Slab(c0, ldc, 12, m * ldc + cpad, CANARY, dev)
        plan = run_gemm(kind, dev, m=m, n=n, k=k, ta=ta, tb=tb, alpha=0.5, beta=0.25, A=A, B=B,
                        C=C, bias=bias.to(dev), batch=batch)
        assert plan.rung == expected_rung(kind, mode, m, n, k, batch), (shape, strides, plan)
        assert not plan.rung.startswith("h3"), plan
        assert plan.main_wgs == 0 and plan.nsplit > 1, plan       # the batched reduce runs
        assert plan.grid == plan.tail_tiles * batch * plan.nsplit, plan
        if kind == "sgemm":
            assert plan.vec == rows16(C), plan
            assert odd or plan.vec == int(strides != "c+1"), plan
        refs = ref64(a, b[:1] if strides == "shared-b" else b, c0, bias, 0.5, 0.25, ta, tb)
        check(C, refs, plan, f"{kind} {shape} {strides} ta{ta} tb{tb}")


# ------------------------------------------------------------------ d. the workspace ladder
@pytest.mark.parametrize("ws,rung,split", [(WS_NONE, "x6_m16_160", False),
                                           (WS_SLABS_LESS_1, "x6_m16_160", False),
                                           (WS_SLABS, "x6_m16_160", True),
                                           (WS_FULL, "h3_160", True)])
def test_workspace_ladder(dev, ws, rung, split, monkeypatch):
    """S under the default switches: without a workspace (ds2_sgemm) or with a byte less than
    the split slabs, whole-K pieces on the bf16x6 kernel; with exactly the slabs, the split on
    the bf16x6 kernel; with the size the query returns, fp16x3.  Each correct at 1e-5."""
    gemm_env(monkeypatch, "h3")
    m, n, k = SHAPES["S"]
    for ta, tb in TRANS:
        a, b, c0, bias = make_inputs("sgemm", m, n, k, ta, tb, 77 + 10 * ta + tb)
        A = operand(a, ta, 8, 4, None, dev)
        B = operand(b, tb, 12, 8, None, dev)
        C = Slab(c0, n + 4, 12, 0, CANARY, dev)
        plan = run_gemm("sgemm", dev, m=m, n=n, k=k, ta=ta, tb=tb, alpha=0.5, beta=0.25, A=A, B=B,
                        C=C, bias=bias.to(dev), ws=ws)
        assert plan.rung == rung and (plan.nsplit > 1) == split, plan
        assert (plan.nsplit, plan.kchunk) == ((4, 256) if split else (1, k)), plan
        check(C, ref64(a, b, c0, bias, 0.5, 0.25, ta, tb), plan, f"ladder {ws} ta{ta} tb{tb}")


# ------------------------------------------------------------------ e. fp16x3 scale edges
def _amax_on_device(X, logical_rows_are_stored_rows, dev):
    """ds2_amax over a padded, offset operand: the maxima of its logical rows."""
    out = torch.zeros(X.rows if logical_rows_are_stored_rows else X.cols, dtype=torch.int32,
                      device=dev)
    r, c = (out.data_ptr(), None) if logical_rows_are_stored_rows else (None, out.data_ptr())
    _lib.call("ds2_amax", X.ptr, X.rows, X.cols, X.ld, r, c, ops._stream())
    return out


def h3_edge_run(dev, name, ta, tb, alpha=1.0, beta=0.0, with_bias=False, claims=True):
    """One fp16x3 GEMM on S with the case's operands (padded, offset, in NaN) and claimed
    maxima.  Returns (plan, C entries, float64 reference of the bare product, bound, keep, c0,
    bias, operands)."""
    m, n, k = SHAPES["S"]
    a, bt, a_claim, b_claim = h3_case(name)
    if not claims:
        a_claim = b_claim = None
    am, bm = h3_maxima(a, bt, a_claim, b_claim)
    ta_, tb_ = torch.from_numpy(a), torch.from_numpy(bt)
    A = operand([ta_.t().contiguous() if ta else ta_], ta, 8, 4, None, dev)
    B = operand([tb_ if tb else tb_.t().contiguous()], tb, 12, 8, None, dev)
    g = torch.Generator().manual_seed(9)
    c0 = torch.randn(m, n, generator=g)
    bias = torch.randn(n, generator=g) if with_bias else None
    C = Slab([c0 if beta != 0.0 else torch.full_like(c0, NAN)], n + 4, 12, 0, CANARY, dev)
    dev_bits = lambda x: None if x is None else torch.from_numpy(bits_of(x).view(np.int32)).to(dev)
    plan = run_gemm("sgemm", dev, m=m, n=n, k=k, ta=ta, tb=tb, alpha=alpha, beta=beta, A=A, B=B,
                    C=C, bias=None if bias is None else bias.to(dev), a_amax=dev_bits(a_claim),
                    b_amax=dev_bits(b_claim))
    assert plan.rung == "h3_160" and (plan.nsplit, plan.kchunk) == (4, 256), plan
    assert plan.amax_passes == int(a_claim is None) + int(b_claim is None), plan
    assert C.outside_unchanged(), plan
    ref = a.astype(np.float64) @ bt.astype(np.float64).T
    return plan, C.read()[0], ref, h3_bound(a, bt, am, bm), normal_range(ref), c0, bias, (A, B)


@pytest.mark.parametrize("name", H3_CASES)
def test_h3_scale_edges(dev, name, monkeypatch):
    """The fp16x3 rung on S at the edges of its row scales, self-computed and caller-supplied
    (ds2_sgemm_amax_ws), all four transposes, operands padded and offset inside NaN.  Element
    by element |C - C64| <= 2^-20 (|A||B|) + 2^-38 (amax_A (x) sum_k |B| + sum_k |A| (x) amax_B)
    with amax the maxima the scales came from (test_gemm_h3_bound_cpu.py derives it and shows
    the inputs meet it in emulation).  zero: a zero row of op(A) and a zero column of op(B)
    give exactly beta * C + bias.  scaled-rows: rows of op(A) scaled by 2^U[-120, 100), the
    scale exponent clamping at 127; outputs whose true value leaves the normal float32 range
    are excluded (none at these inputs; under 1 % asserted).  loose-e: claimed maxima 2^e
    times the true ones on both operands (2^20 is asserted against the bound only; its figures
    are recorded in profiles/gemm_h3_loose_bound.jsonl).  unit-bound: the bound 1.0 for an
    operand of magnitude 1e-2, as dW_hh passes for h.  spike-d: column 0 of op(A) times 2^d
    against a zero row of op(B) -- at d = 24 the elements 2^17 and more below the row maximum
    lose bits and the plain componentwise error leaves the 1e-6 bar (5e-6 in emulation) while
    the bound holds.  loose-0: exact maxima, from ds2_amax on the padded operands, give the
    bits of the kernel's own pre-pass."""
    gemm_env(monkeypatch, "h3")
    for ta, tb in TRANS:
        if name == "zero":
            plan, got, ref, bound, keep, c0, bias, _ = h3_edge_run(dev, name, ta, tb, 0.5, 0.25,
                                                                   True)
            exact = 0.25 * c0 + bias
            assert torch.equal(got[5, :], exact[5, :]) and torch.equal(got[:, 7], exact[:, 7])
            assert torch.isfinite(got).all().item()
            close(got, 0.5 * torch.from_numpy(ref) + 0.25 * c0.double() + bias.double(), 1e-5,
                  f"h3 zero ta{ta} tb{tb}")
            continue
        plan, got, ref, bound, keep, _, _, (A, B) = h3_edge_run(dev, name, ta, tb)
        assert 1.0 - keep.mean() < 0.01
        got = got.double().numpy()
        assert np.isfinite(got[keep]).all(), (name, ta, tb)
        err = np.abs(got - ref)
        worst = np.where(keep, err - bound, -1.0).max()
        ratio = np.where(keep & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0).max()
        print(f"h3 {name} ta{ta} tb{tb}: max err / bound {ratio:.4f}, excluded "
              f"{1.0 - keep.mean():.4%}")
        assert worst <= 0.0, (name, ta, tb, ratio)
        if name == "loose-0":
            _, own, *_ = h3_edge_run(dev, name, ta, tb, claims=False)
            assert np.array_equal(own.double().numpy(), got), (ta, tb)
            a, bt, a_claim, b_claim = h3_case(name)
            ra = _amax_on_device(A, not ta, dev).cpu().numpy().view(np.uint32)
            rb = _amax_on_device(B, bool(tb), dev).cpu().numpy().view(np.uint32)
            assert np.array_equal(ra, bits_of(a_claim)) and np.array_equal(rb, bits_of(b_claim))
