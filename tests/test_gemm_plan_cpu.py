"""CPU: the GEMM family's host selection (csrc/gemm_host.h gemm_select) and its work decode.

ds2_test_sgemm_plan returns what ds2_sgemm* / ds2_sgemm_bf16_ws / ds2_bgemm_nt would launch
(the function the entry points switch on, nothing recomputed); ds2_test_sgemm_cover runs every
workgroup id of that grid through the kernels' own decode_work / tile_coords / bg_decode on the
host.  No device: the CU count is an argument.  The properties below follow from the code and
from the header's promises, not from recorded outputs.
"""
import itertools

import pytest

import torch  # noqa: F401  (load torch's HIP runtime first: one libamdhip64 per process)
from ds2amd import _lib, ops

MN = (1, 37, 128, 129, 256, 257, 300, 2400, 16032)
KS = (1, 4, 31, 32, 36, 255, 256, 512, 1021, 1024, 1028, 5000, 16032)
BATCHES = (1, 3)
CUS = (8, 64, 256, 304)
# (DS2_GEMM_X6, DS2_GEMM_H3); None: unset
SWITCHES = {"default": (None, None), "h3_off": (None, "0"), "x6_off": ("0", None)}
BIG = 1 << 44            # a workspace no plan outgrows

H3 = ("h3_160", "h3_128")
X6 = ("x6_m16_160", "x6_m16_128", "x6_160", "x6_128", "x6_k_160", "x6_k_128")
X6_K = ("x6_k_160", "x6_k_128")
# k per stage and resident workgroups per CU of each rung's kernel
STAGE = dict({r: 32 for r in H3 + X6}, f64_160=64, f64_128=64, f16=16, bf16_staged=64,
             bf16_dma=64, bf16_dma_k=64)
PER_CU = dict({r: 1 for r in H3 + X6}, f64_160=2, f64_128=2, f16=3, bf16_staged=2, bf16_dma=1,
              bf16_dma_k=1)


def _env(monkeypatch, switches):
    for name, v in zip(("DS2_GEMM_X6", "DS2_GEMM_H3"), SWITCHES[switches]):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _up4(x):
    return (x + 3) // 4 * 4


def _call(kind, m, n, k, batch, aligned):
    """Keyword arguments of ops.gemm_plan for one call of the sweep.  aligned: 16-byte
    addresses, leading dimensions and strides that are multiples of 4, plain operands;
    else both operands transposed at an address 4 bytes off."""
    if kind == "bgemm_nt":
        ld = (k + 7) // 8 * 8 + (0 if aligned else 4)
        return dict(m=m, n=n, k=k, lda=ld, ldb=ld, ldc=n)
    if aligned:
        lda, ldb = _up4(k), _up4(n)
        return dict(m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=_up4(n), stride_a=m * lda,
                    stride_b=k * ldb, stride_c=m * _up4(n), batch=batch)
    return dict(m=m, n=n, k=k, trans_a=True, trans_b=True, a=260, b=260, c=260, lda=m, ldb=k,
                ldc=n, stride_a=m * k, stride_b=n * k, stride_c=m * n, batch=batch)


def _staged4(kw):
    """Both operands can be staged as float4 (gemm_select's va and vb)."""
    if kw.get("a", 256) % 16 or kw.get("b", 256) % 16:
        return False
    if kw["lda"] % 4 or kw["ldb"] % 4 or kw.get("stride_a", 0) % 4 or kw.get("stride_b", 0) % 4:
        return False
    ea = kw["m"] if kw.get("trans_a") else kw["k"]
    eb = kw["k"] if kw.get("trans_b") else kw["n"]
    return ea % 4 == 0 and eb % 4 == 0


def _check_plan(kind, kw, p, cus, switches):
    m, n, k, batch = kw["m"], kw["n"], kw["k"], kw.get("batch", 1)
    what = (kind, kw, p, cus, switches)
    assert p.status == 0 and p.rung != "none", what
    tiles = -(-m // p.bm) * -(-n // p.bn)
    assert p.nsplit >= 1 and (p.nsplit - 1) * p.kchunk < k <= p.nsplit * p.kchunk, what
    if p.nsplit > 1:
        assert p.kchunk % STAGE[p.rung] == 0, what
    if batch == 1:
        assert p.main_wgs + p.tail_tiles == tiles, what
    else:
        assert p.main_wgs == 0 and p.tail_tiles == tiles, what
    assert p.main_wgs % (PER_CU[p.rung] * cus) == 0, what
    assert p.tail_tile0 == p.main_wgs, what
    assert p.grid == p.main_wgs + p.tail_tiles * batch * p.nsplit, what
    assert ops.gemm_cover(m, n, k, batch, p) == 0, what
    # rung consistency
    staged4 = kind == "bgemm_nt" or _staged4(kw)
    x6_off = SWITCHES[switches][0] == "0"
    if kind == "sgemm":
        if p.rung in H3:
            assert staged4 and k % 32 == 0 and batch == 1 and not x6_off, what
            assert p.nsplit == 1 or p.kchunk % 32 == 0, what
            assert SWITCHES[switches][1] != "0", what
        if not staged4:
            assert p.rung == "f16", what
        elif x6_off:
            assert p.rung in ("f64_160", "f64_128"), what
        elif k % 32:
            assert p.rung in X6_K, what                     # a K tail: the k-checked rung
        else:
            assert p.rung in H3 + X6, what
        assert (p.bm, p.bn) == dict({r: (256, int(r[-3:])) for r in H3 + X6}, f64_160=(128, 160),
                                    f64_128=(128, 128), f16=(128, 128))[p.rung], what
    elif kind == "sgemm_bf16":
        assert p.rung == "bf16_staged" and (p.bm, p.bn) == (128, 128), what
    else:
        assert p.rung == ("bf16_dma_k" if k % 64 else "bf16_dma"), what
        assert (p.bm, p.bn) == (256, 256), what


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("aligned", (True, False), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("switches", list(SWITCHES))
@pytest.mark.parametrize("kind", ops.GEMM_KINDS)
def test_plan_sweep(monkeypatch, kind, switches, aligned, cus):
    """Every plan of the grid is well formed, its decode covers every (batch, tile) x [0, K)
    exactly once, and its rung is the one the call's alignment, K tail and switches allow."""
    if kind != "sgemm" and switches != "default":
        return                      # the switches are the fp32 family's: nothing else reads them
    _env(monkeypatch, switches)
    for m, n, k, batch in itertools.product(MN, MN, KS, BATCHES):
        if kind == "bgemm_nt" and batch != 1:
            continue
        kw = _call(kind, m, n, k, batch, aligned)
        p = ops.gemm_plan(kind, ws_bytes=BIG, cus=cus, **kw)
        if kind == "sgemm_bf16" and not _staged4(kw):
            assert (p.status, p.rung) == (_lib.UNSUPPORTED_SHAPE, "none"), (kw, p)
            continue
        if kind == "bgemm_nt" and (k % 8 or not aligned):
            assert (p.status, p.rung) == (_lib.UNSUPPORTED_SHAPE, "none"), (kw, p)
            continue
        _check_plan(kind, kw, p, cus, switches)


@pytest.mark.parametrize("aligned", (True, False), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("switches", list(SWITCHES))
def test_workspace_queries_cover_every_rung(monkeypatch, switches, aligned):
    """The header's promise: ds2_sgemm_workspace_size is "large enough for any kernel's plan",
    whatever the alignment and the switches -- and with exactly that much the plan is the one
    an unbounded workspace gets.  The same for the bf16 and bgemm queries.  (cus = 0: the
    queries plan for the current device, 256 CUs where there is none.)"""
    _env(monkeypatch, switches)
    for m, n, k, batch in itertools.product(MN, MN, KS, BATCHES):
        for kind in ops.GEMM_KINDS:
            if kind == "bgemm_nt":
                if batch != 1:
                    continue
                size = _lib.size("ds2_bgemm_workspace_size", m, n, k)
            else:
                size = _lib.size("ds2_" + kind + "_workspace_size", m, n, k, batch)
            kw = _call(kind, m, n, k, batch, aligned)
            full = ops.gemm_plan(kind, ws_bytes=BIG, **kw)
            got = ops.gemm_plan(kind, ws_bytes=size or None, **kw)
            assert full.ws_bytes <= size, (kind, kw, full, size)
            assert got == full, (kind, kw, got, full, size)


def test_no_workspace_ladder(monkeypatch):
    """Without a workspace, or with one byte less than the split slabs, every plan is unsplit
    and never fp16x3; with exactly the slabs it is split but not fp16x3; fp16x3 needs the
    row-scale words ((m + n) * 4 + 512 bytes) after the slabs."""
    _env(monkeypatch, "default")
    seen_split_h3 = 0
    for m, n, k, batch, cus in itertools.product(MN, MN, KS, BATCHES, CUS):
        for kind in ("sgemm", "sgemm_bf16"):
            kw = _call(kind, m, n, k, batch, True)
            if not _staged4(kw):
                continue
            full = ops.gemm_plan(kind, ws_bytes=BIG, cus=cus, **kw)
            none = ops.gemm_plan(kind, ws_bytes=None, cus=cus, **kw)
            assert none.nsplit == 1 and none.kchunk == k and none.rung not in H3, (kw, none)
            assert none.ws_bytes == 0 and none.grid == none.main_wgs + none.tail_tiles * batch
            assert ops.gemm_cover(m, n, k, batch, none) == 0, (kw, none)
            # without the scale words a workspace pointer alone does not make it fp16x3
            assert ops.gemm_plan(kind, ws_bytes=0, cus=cus, **kw) == none, (kw, none)
            if full.nsplit == 1:
                continue
            scale_words = (m + n) * 4 + 512 if full.rung in H3 else 0
            slabs = full.ws_bytes - scale_words
            assert slabs == full.nsplit * batch * full.tail_tiles * full.bm * full.bn * 4 + 256
            short = ops.gemm_plan(kind, ws_bytes=slabs - 1, cus=cus, **kw)
            assert short == none, (kw, short, none)
            exact = ops.gemm_plan(kind, ws_bytes=slabs, cus=cus, **kw)
            assert exact.rung not in H3 and exact.ws_bytes == slabs, (kw, exact)
            assert (exact.nsplit, exact.kchunk, exact.grid) == (full.nsplit, full.kchunk,
                                                                full.grid), (kw, exact, full)
            if full.rung in H3:
                seen_split_h3 += 1
                assert exact.rung == full.rung.replace("h3", "x6_m16"), (kw, exact, full)
                one_short = ops.gemm_plan(kind, ws_bytes=full.ws_bytes - 1, cus=cus, **kw)
                assert one_short == exact, (kw, one_short)
    assert seen_split_h3 > 100


def test_worked_examples_at_256_cus(monkeypatch):
    """The two examples of the GemmPlan comment (csrc/gemm_host.h)."""
    _env(monkeypatch, "default")
    # the input projection's 16032 x 2400 on the BK=16 kernel's 128-wide tiles (an operand off
    # 16-byte alignment): 19 * 126 = 2394 tiles = 3 rounds of 768 + 90 tail tiles
    p = ops.gemm_plan("sgemm", m=16032, n=2400, k=2048, a=260, lda=2048, ldb=2400, ldc=2400,
                      ws_bytes=BIG, cus=256)
    assert (p.rung, p.bm, p.bn) == ("f16", 128, 128)
    assert (p.main_wgs, p.tail_tile0, p.tail_tiles) == (3 * 768, 3 * 768, 90)
    assert (p.nsplit, p.kchunk, p.grid) == (8, 256, 2304 + 90 * 8)
    assert ops.gemm_cover(16032, 2400, 2048, 1, p) == 0
    # the weight gradient 2400 x 800, K = 16032 (dW = dG^T X): fp16x3 on 256 x 160 tiles,
    # 10 * 5 = 50 tiles, no whole round, 5 splits of 3232 k (101 stages of 32)
    p = ops.gemm_plan("sgemm", m=2400, n=800, k=16032, trans_a=True, lda=2400, ldb=800, ldc=800,
                      ws_bytes=BIG, cus=256)
    assert (p.rung, p.bm, p.bn) == ("h3_160", 256, 160)
    assert (p.main_wgs, p.tail_tiles, p.nsplit, p.kchunk, p.grid) == (0, 50, 5, 3232, 250)
    assert p.ws_bytes == 5 * 50 * 256 * 160 * 4 + 256 + (2400 + 800) * 4 + 512
    assert p.amax_passes == 2
    assert ops.gemm_cover(2400, 800, 16032, 1, p) == 0


def test_cover_sees_a_broken_plan():
    """The cover check is not vacuous: a plan whose pieces overlap, leave a K gap, miss a tile
    or fall outside the tile grid is counted."""
    p = ops.gemm_plan("sgemm", m=300, n=260, k=1024, lda=1024, ldb=260, ldc=260, ws_bytes=BIG,
                      cus=256)
    assert p.nsplit == 4 and p.tail_tiles == 4 and ops.gemm_cover(300, 260, 1024, 1, p) == 0
    # whole tiles 0-3 and the pieces of tiles 0-3 as well: every tile covered twice
    assert ops.gemm_cover(300, 260, 1024, 1, p._replace(main_wgs=4, grid=p.grid + 4)) == 4
    assert ops.gemm_cover(300, 260, 1024, 1, p._replace(kchunk=p.kchunk - 32)) == 4   # gap
    # split 3 decodes as batch entry 1 (4 outside), and the other three end at 768 (4 gaps)
    assert ops.gemm_cover(300, 260, 1024, 1, p._replace(nsplit=3)) == 8
    assert ops.gemm_cover(300, 260, 1024, 1, p._replace(grid=p.grid - 1)) >= 1        # a piece
    assert ops.gemm_cover(300, 260, 1024, 1, p._replace(tail_tile0=1)) >= 1           # outside
    assert ops.gemm_cover(300, 260, 1024, 2, p) >= 4                                  # batch 1
    assert ops.gemm_cover(0, 260, 1024, 1, p) == -1


def test_rejections_before_any_launch():
    """Host-side argument checks, through the entry points themselves with null operands
    (they return before any launch): ld below the extent and negative sizes are
    DS2_INVALID_VALUE; an empty product is DS2_OK; K = 0 with m, n > 0 is
    DS2_UNSUPPORTED_SHAPE (the split-operand kernels load their first stage before they test
    the K range), as are bf16 operands that cannot be staged as float4."""
    lib = _lib.load()

    def ws(m, n, k, lda, ldb, ldc, batch=1, ta=0, tb=0, fn="ds2_sgemm_ws", a=None, b=None):
        return getattr(lib, fn)(ta, tb, m, n, k, 1.0, a, lda, 0, b, ldb, 0, 0.0, None, ldc, 0,
                                batch, None, None, 0, None)

    for fn in ("ds2_sgemm_ws", "ds2_sgemm_bf16_ws"):
        assert ws(4, 4, 4, 3, 4, 4, fn=fn) == 1          # lda < k
        assert ws(4, 4, 4, 3, 4, 4, ta=1, fn=fn) == 1    # lda < m
        assert ws(4, 4, 4, 4, 3, 4, fn=fn) == 1          # ldb < n
        assert ws(4, 4, 4, 4, 4, 3, fn=fn) == 1          # ldc < n
        assert ws(4, 4, 4, 4, 4, 4, batch=-1, fn=fn) == 1
        assert ws(4, 4, -1, 4, 4, 4, fn=fn) == 1
        assert ws(0, 4, 4, 4, 4, 4, fn=fn) == 0
        assert ws(4, 4, 4, 4, 4, 4, batch=0, fn=fn) == 0
        assert ws(4, 4, 0, 4, 4, 4, fn=fn) == _lib.UNSUPPORTED_SHAPE
    assert ws(4, 4, 4, 4, 4, 4, fn="ds2_sgemm_bf16_ws", a=4) == _lib.UNSUPPORTED_SHAPE
    assert ws(4, 4, 4, 5, 4, 4, fn="ds2_sgemm_bf16_ws") == _lib.UNSUPPORTED_SHAPE
    assert lib.ds2_sgemm(0, 0, 4, 4, 0, 1.0, None, 4, 0, None, 4, 0, 0.0, None, 4, 0, 1, None,
                         None) == _lib.UNSUPPORTED_SHAPE
    assert lib.ds2_sgemm_amax_ws(0, 0, 4, 4, 0, 1.0, None, 4, None, 4, 0.0, None, 4, None, None,
                                 None, None, 0, None) == _lib.UNSUPPORTED_SHAPE
    # ds2_bgemm_nt: null operands and short ld are invalid, k % 8, ld % 8 and K = 0 unsupported
    def bg(m, n, k, lda, ldb, ldc, a=256, b=256, c=256):
        return lib.ds2_bgemm_nt(m, n, k, 1.0, a, lda, b, ldb, 0.0, c, ldc, None, None, 0, None)

    assert bg(8, 8, 8, 8, 8, 8, a=None) == 1
    assert bg(8, 8, 8, 0, 8, 8) == 1
    assert bg(8, 8, 8, 8, 8, 4) == 1
    assert bg(8, 8, -8, 8, 8, 8) == 1
    assert bg(0, 8, 8, 8, 8, 8) == 0
    assert bg(8, 8, 4, 8, 8, 8) == _lib.UNSUPPORTED_SHAPE
    assert bg(8, 8, 8, 12, 8, 8) == _lib.UNSUPPORTED_SHAPE
    assert bg(8, 8, 8, 8, 8, 8, a=264) == _lib.UNSUPPORTED_SHAPE
    assert bg(8, 8, 0, 8, 8, 8) == _lib.UNSUPPORTED_SHAPE
    # the plan hook reports the same statuses
    assert ops.gemm_plan("sgemm", m=4, n=4, k=0, lda=4, ldb=4, ldc=4).status == 2
    assert ops.gemm_plan("sgemm", m=4, n=4, k=4, lda=3, ldb=4, ldc=4).status == 1
    assert ops.gemm_plan("sgemm", m=0, n=4, k=4, lda=4, ldb=4, ldc=4)[:2] == ("none", 0)
