"""Helpers of the GEMM contract tests (test_gpu_gemm_contract.py, test_gemm_h3_bound_cpu.py):
operands placed inside larger, poisoned allocations, the C entry points called directly with
every argument of the ABI (offsets, leading dimensions, batch strides, workspace size), the
library's own plan for exactly that call, and float64 references."""
import numpy as np
import torch

from ds2amd import _lib, ops

# the smallest shapes at which each tiling has two tile rows and two tile columns with partial
# edges and an eligible K split (k / 256 = 4)
SHAPES = {
    "S": (300, 260, 1024),          # 256 x 160 tiles (n >= 256), every stage inside K
    "S-narrow": (300, 200, 1024),   # 256 x 128 tiles
    "S-ktail": (300, 260, 1028),    # a K tail: the k-checked 32x32x16 form
    "S-ktail-narrow": (300, 200, 1028),
    "S-odd": (301, 259, 1021),      # not float4-stageable: the BK=16 fp32 kernel
    "S-ktail8": (300, 260, 1032),   # bf16 operands (k % 8 == 0) with a masked last K-tile
}
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]

CANARY = 0x5CA1AB1E   # the word every element of a C allocation outside the matrix holds


def gemm_env(monkeypatch, mode):
    """h3: the default (fp16x3 where it can run); x6: DS2_GEMM_H3=0 (bf16x6); fp32:
    DS2_GEMM_X6=0 (the fp32-MFMA kernels)."""
    monkeypatch.setenv("DS2_GEMM_X6", "0" if mode == "fp32" else "1")
    monkeypatch.setenv("DS2_GEMM_H3", "1" if mode == "h3" else "0")


class Slab:
    """`mats` ([rows][cols] CPU tensors, one per batch entry) stored row-major with leading
    dimension ld at element offset off + b * stride of one allocation; every other element
    of the allocation holds `fill` (a float, or an int32 bit pattern).  The allocation ends
    rows * ld + 64 elements after the last entry's start, so the whole rows x ld span a
    kernel may address lies inside it."""

    def __init__(self, mats, ld, off, stride, fill, dev):
        self.rows, self.cols = mats[0].shape
        self.ld, self.off, self.stride, self.nb = ld, off, stride, len(mats)
        assert ld >= self.cols and off >= 0
        assert self.nb == 1 or stride >= (self.rows - 1) * ld + self.cols   # entries disjoint
        self.dtype = mats[0].dtype
        size = off + (self.nb - 1) * stride + self.rows * ld + 64
        if isinstance(fill, int):
            host = torch.full((size,), fill, dtype=torch.int32).view(self.dtype)
        else:
            host = torch.full((size,), fill, dtype=self.dtype)
        self.mask = torch.zeros(size, dtype=torch.bool)
        within = torch.arange(self.rows)[:, None] * ld + torch.arange(self.cols)[None, :]
        self.index = [off + b * stride + within for b in range(self.nb)]
        for idx, mt in zip(self.index, mats):
            assert not self.mask[idx].any()
            host[idx] = mt
            self.mask[idx] = True
        self.before = host.clone()
        self.buf = host.to(dev)
        self.es = self.buf.element_size()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.es * self.off

    def read(self):
        """The batch entries as they are on the device now."""
        host = self.buf.cpu()
        return [host[idx] for idx in self.index]

    def outside_unchanged(self):
        """Every word outside the matrices is bit-identical to what was put there."""
        now = self.buf.cpu().view(torch.int32)[~self.mask]
        return torch.equal(now, self.before.view(torch.int32)[~self.mask])


def rows16(C):
    """Every row of every batch entry of C starts 16-byte aligned (the 16-byte form of the
    split reduce needs it; the tests' bias vectors are fresh allocations, always aligned)."""
    return int(C.ptr % 16 == 0 and C.ld % 4 == 0 and C.stride % 4 == 0)


def operand(mats, trans, pad, off, stride_pad, dev, nb=1, fill=float("nan"), wide=False):
    """An A or B operand: logical [r][c] matrices stored as given (trans: stored transposed is
    the caller's business -- `mats` are the STORED matrices).  ld = cols + pad; wide: the
    model's form, the right half of a twice as wide buffer (ld = 2 cols, off += cols).
    stride_pad None: one shared entry (stride 0)."""
    rows, cols = mats[0].shape
    ld = 2 * cols if wide else cols + pad
    off = off + (cols if wide else 0)
    if stride_pad is None:
        return Slab(mats[:1], ld, off, 0, fill, dev)
    return Slab(mats, ld, off, rows * ld + stride_pad, fill, dev)


def ref64(a_mats, b_mats, c_mats, bias, alpha, beta, ta, tb):
    """alpha op(A) op(B) + beta C + bias per batch entry, in float64 on the CPU, from the
    stored operands (a shared operand: a list of one)."""
    out = []
    for i, c0 in enumerate(c_mats):
        a = a_mats[min(i, len(a_mats) - 1)].double()
        b = b_mats[min(i, len(b_mats) - 1)].double()
        r = alpha * ((a.t() if ta else a) @ (b.t() if tb else b))
        if beta != 0.0:
            r = r + beta * c0.double()
        if bias is not None:
            r = r + bias.double()
        out.append(r)
    return out


def close(got, ref, rel=1e-5, name=""):
    """The project's GEMM bar: max |got - ref| <= rel * max |ref|."""
    got, ref = got.double(), ref.double()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


WS_FULL, WS_NONE, WS_SLABS, WS_SLABS_LESS_1 = "full", "none", "slabs", "slabs-1"


def run_gemm(kind, dev, *, m, n, k, ta, tb, alpha, beta, A, B, C, bias, batch=1, ws=WS_FULL,
             a_amax=None, b_amax=None):
    """One call of the C entry point (ds2_sgemm_ws / ds2_sgemm / ds2_sgemm_amax_ws for kind
    "sgemm", ds2_sgemm_bf16_ws, ds2_bgemm_nt) on Slab operands.  Returns the library's plan for
    exactly this call (ds2_test_sgemm_plan with cus = 0, asked before the launch).  ws: the
    full size the query returns, none (ds2_sgemm), exactly the split slabs, or a byte less."""
    stream = ops._stream()
    if kind == "bgemm_nt":
        size = _lib.size("ds2_bgemm_workspace_size", m, n, k)
    else:
        size = _lib.size("ds2_" + kind + "_workspace_size", m, n, k, batch)
    common = dict(m=m, n=n, k=k, trans_a=ta, trans_b=tb, a=A.ptr, lda=A.ld, stride_a=A.stride,
                  b=B.ptr, ldb=B.ld, stride_b=B.stride, c=C.ptr, ldc=C.ld, stride_c=C.stride,
                  batch=batch, bias=0 if bias is None else bias.data_ptr(),
                  amax_given=int(a_amax is not None) | 2 * int(b_amax is not None))
    full = ops.gemm_plan(kind, ws_bytes=size or None, **common)
    if ws == WS_FULL:
        nbytes = size
    elif ws == WS_NONE:
        nbytes = None
    else:
        scale_words = (m + n) * 4 + 512 if full.rung.startswith("h3") else 0
        nbytes = full.ws_bytes - scale_words - (1 if ws == WS_SLABS_LESS_1 else 0)
        assert full.nsplit > 1 and nbytes > 0
    plan = ops.gemm_plan(kind, ws_bytes=nbytes or None, **common)
    assert plan.status == 0 and plan.rung != "none", plan
    assert plan.ws_bytes <= (nbytes or 0)
    wsbuf = None if not nbytes else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    wp, wn = (None, 0) if wsbuf is None else (wsbuf.data_ptr(), nbytes)
    bp = None if bias is None else bias.data_ptr()
    if kind == "bgemm_nt":
        assert batch == 1 and not ta and tb
        _lib.call("ds2_bgemm_nt", m, n, k, alpha, A.ptr, A.ld, B.ptr, B.ld, beta, C.ptr, C.ld, bp,
                  wp, wn, stream)
    elif a_amax is not None or b_amax is not None:
        assert kind == "sgemm" and batch == 1
        _lib.call("ds2_sgemm_amax_ws", ta, tb, m, n, k, alpha, A.ptr, A.ld, B.ptr, B.ld, beta,
                  C.ptr, C.ld, bp, None if a_amax is None else a_amax.data_ptr(),
                  None if b_amax is None else b_amax.data_ptr(), wp, wn, stream)
    elif ws == WS_NONE and kind == "sgemm":
        _lib.call("ds2_sgemm", ta, tb, m, n, k, alpha, A.ptr, A.ld, A.stride, B.ptr, B.ld,
                  B.stride, beta, C.ptr, C.ld, C.stride, batch, bp, stream)
    else:
        _lib.call("ds2_" + kind + "_ws", ta, tb, m, n, k, alpha, A.ptr, A.ld, A.stride, B.ptr,
                  B.ld, B.stride, beta, C.ptr, C.ld, C.stride, batch, bp, wp, wn, stream)
    torch.cuda.synchronize()
    return plan


# ---------------------------------------------------------------------------------------------
# The fp16x3 error model (csrc/split_mma.h split_store8<2> and h3_exp), in NumPy.

def h3_exp(amax_bits):
    """The row-scale exponent of a claimed row maximum (float bits), as split_mma.h h3_exp."""
    bits = np.asarray(amax_bits, dtype=np.uint32)
    E = (bits >> 23).astype(np.int64)
    e = 14 - (np.where(E == 0, 1, E) - 127)
    e = np.minimum(e, 127)
    return np.where((bits == 0) | (E >= 255), 0, e)


def bits_of(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def h3_split(x, amax_bits):
    """fp16 (hi, lo) of the rows of x scaled by 2^e, e from the claimed row maxima: hi =
    fp16(x 2^e), lo = fp16(x 2^e - hi), as float64 values, and e."""
    e = h3_exp(amax_bits)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.ldexp(x.astype(np.float64), e).astype(np.float32)   # exact: a power of two
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), e


def h3_emulate(a, b, a_amax_bits, b_amax_bits):
    """op(A) [m][k] x op(B)^T ([n][k] rows) as the fp16x3 kernel forms it: hi*hi + hi*lo +
    lo*hi of the row-scaled fp16 splits with exact products (float64 sums stand in for the
    fp32 accumulator, whose rounding the fp32-MFMA kernel shares), scaled back."""
    ah, al, ea = h3_split(a, a_amax_bits)
    bh, bl, eb = h3_split(b, b_amax_bits)
    acc = ah @ bh.T + ah @ bl.T + al @ bh.T
    return np.ldexp(acc, -(ea + eb.T))


def h3_bound(a, b, alpha_max, beta_max):
    """The element-wise bound of the issue: 2^-20 |A||B| + 2^-38 (amax_A (x) sum_k |B| +
    sum_k |A| (x) amax_B), from the staging error max(2^-22 |x|, 2^-39 claimed max) of each
    element and the dropped lo*lo term (< 2^-22 |ab|), with a factor 2."""
    a, b = np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))
    am = np.asarray(alpha_max, dtype=np.float64)[:, None]
    bm = np.asarray(beta_max, dtype=np.float64)[None, :]
    return 2.0 ** -20 * (a @ b.T) + 2.0 ** -38 * (am * b.sum(1)[None, :] + a.sum(1)[:, None] * bm)


# The fp16x3 scale-edge inputs on S (m, n, k = 300, 260, 1024): name -> builder.  Each gives
# op(A) [m][k], op(B)^T [n][k] (float32 NumPy), and the row maxima the caller claims for each
# (None: the kernel's own pre-pass, i.e. the exact maxima).
H3_LOOSE = (0, 8, 16, 20)          # claimed maxima 2^e times the true ones; 20: recorded too
H3_SPIKES = (10, 17, 24)
H3_CASES = (["zero", "scaled-rows", "unit-bound"] + ["loose-%d" % e for e in H3_LOOSE]
            + ["spike-%d" % d for d in H3_SPIKES])


def h3_case(name, seed=3):
    m, n, k = SHAPES["S"]
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    a = rng.standard_normal((m, k)).astype(np.float32)
    bt = rng.standard_normal((n, k)).astype(np.float32)
    a_claim = b_claim = None
    if name == "zero":                       # a zero row of op(A), a zero column of op(B)
        a[5, :] = 0.0
        bt[7, :] = 0.0
    elif name == "scaled-rows":              # rows of op(A) scaled by 2^U[-120, 100)
        a = np.ldexp(a, rng.integers(-120, 100, size=(m, 1))).astype(np.float32)
    elif name == "unit-bound":               # |h| < 1 of magnitude 1e-2 under the bound 1.0
        bt = np.clip(bt * np.float32(1e-2), -0.999, 0.999).astype(np.float32)
        b_claim = np.ones(n, dtype=np.float32)
    elif name.startswith("loose-"):
        e = int(name.split("-")[1])
        a_claim = np.ldexp(np.abs(a).max(1), e).astype(np.float32)
        b_claim = np.ldexp(np.abs(bt).max(1), e).astype(np.float32)
    elif name.startswith("spike-"):          # column 0 of op(A) times 2^d, row 0 of op(B) zero
        a[:, 0] = np.ldexp(a[:, 0], int(name.split("-")[1]))
        bt[:, 0] = 0.0
    else:
        raise KeyError(name)
    return a, bt, a_claim, b_claim


def h3_maxima(a, bt, a_claim, b_claim):
    """The row maxima the scales come from: the claimed ones, else the exact ones."""
    am = np.abs(a).max(1) if a_claim is None else a_claim
    bm = np.abs(bt).max(1) if b_claim is None else b_claim
    return am.astype(np.float32), bm.astype(np.float32)


def normal_range(ref):
    """Outputs whose true value lies in the normal float32 range (or is exactly 0)."""
    r = np.abs(ref)
    return (r == 0) | ((r >= 2.0 ** -126) & (r <= float(np.finfo(np.float32).max)))
