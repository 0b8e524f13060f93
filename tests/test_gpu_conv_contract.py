"""GPU: the Conv2d kernels (csrc/conv.hip, csrc/conv_split.hip) against float64 across the
calling contract of ds2_conv2d_fwd / _dgrad / _wgrad: every rung of the dispatch at its tile,
channel-block and row-pairing edges (conv_common.CASES; test_conv_contract_cpu.py proves the
table reaches them all), operands inside poisoned allocations, a workspace of exactly the
plan's size with canaries behind it, MaskConv lengths at their edges, zero and non-finite
samples under the fp16x3 scales, streaming's one- and two-column windows, dgrad positions no
tap reaches, the status codes, and operands that are 4-byte aligned only.

Every bound is the project's conv bound, max |err| <= 1e-5 * max |ref|; conv_common.close
prints each error as a fraction of it (pytest -s)."""
import pytest
import torch

from ds2amd import _lib

from conv_common import (CASES, STREAMING, LEAD4, LEAD16, WS_LEAD, Poisoned, Workspace, assert_rungs,
                         case_settings, close, out_hw, ref64, run_dgrad, run_fwd, run_wgrad,
                         set_env, with_n)

pytestmark = pytest.mark.gpu

OK, INVALID_VALUE, WORKSPACE_TOO_SMALL = 0, 1, 5


def _ids(pairs):
    return [f"{c}-{s}" for c, s in pairs]


def _run_all(cfg, want, dev, name, lead=LEAD16):
    """Forward with bias, dgrad and wgrad with dbias of the directions `want` names, in poison,
    against ref64(cfg); wgrad twice on workspaces that held 0xFF and 0x00."""
    r = ref64(cfg)
    w, b = Poisoned(r.w, dev, lead), Poisoned(r.b, dev, lead)
    x, dy = Poisoned(r.x, dev, lead), Poisoned(r.dy, dev, lead)
    if want[0]:
        y, _, intact = run_fwd(cfg, x, w, b, dev, lead=lead)
        close(y, r.y, name=f"{name} fwd {want[0]}")
        assert intact, f"{name}: a write outside y or past the forward plan's workspace"
    if want[1]:
        dx, _, intact = run_dgrad(cfg, dy, w, dev, lead=lead)
        close(dx, r.dx, name=f"{name} dgrad {want[1]}")
        assert intact, f"{name}: a write outside dx or past the dgrad plan's workspace"
    if want[2]:
        (dw, db), _, intact = run_wgrad(cfg, dy, x, dev, lead=lead)
        close(dw, r.dw, name=f"{name} wgrad {want[2]}")
        close(db, r.db, name=f"{name} dbias")
        assert intact, f"{name}: a write outside dw / dbias or past the wgrad plan's workspace"
        (dw0, db0), _, intact = run_wgrad(cfg, dy, x, dev, lead=lead, ws_fill=0x00)
        assert intact
        assert torch.equal(dw.view(torch.int32), dw0.view(torch.int32)), \
            f"{name}: dw depends on what the workspace held"
        assert torch.equal(db.view(torch.int32), db0.view(torch.int32))


def test_the_poison_shows_a_stray_write(dev):
    """The checks below are live: one word written just before or just behind an output, or
    just behind the workspace, is reported; a write inside is not."""
    for at in (LEAD16 - 1, LEAD16 + 6):
        out = Poisoned((2, 3), dev)
        assert out.intact() and torch.isnan(out.read()).all()
        out.view.fill_(1.0)
        assert out.intact()
        out.buf[at] = 0.0
        assert not out.intact()
    for at in (WS_LEAD - 1, WS_LEAD + 1000):
        ws = Workspace(1000, dev)
        assert ws.ptr % 256 == 0 and ws.intact()
        ws.buf[WS_LEAD:WS_LEAD + 1000] = 0
        assert ws.intact()
        ws.buf[at] = 0
        assert not ws.intact()


@pytest.mark.parametrize("case,setting", case_settings(), ids=_ids(case_settings()))
def test_rung_in_poison(dev, monkeypatch, case, setting):
    """Each rung on operands surrounded by NaN, outputs pre-filled with NaN and surrounded by
    canaries, a 0xFF-filled workspace of exactly the plan's bytes with canaries behind it:
    within 1e-5 of float64, every canary intact, and dw bit-equal when the workspace held
    zeros instead (stale maxima, partial slabs not fully written, a fixed summation order)."""
    set_env(monkeypatch, setting)
    cfg, rungs = CASES[case]
    assert_rungs(cfg, rungs[setting])
    _run_all(cfg, rungs[setting], dev, f"{case}-{setting}")


# (case, setting, the forward rung's column tile)
LENS_CASES = [("A", "default", 256), ("A", "one_row", 256), ("A", "fp32", 128), ("G", "default", 128),
              ("J2", "default", 128), ("H", "default", 256)]


@pytest.mark.parametrize("case,setting,tile", LENS_CASES, ids=[f"{c}-{s}" for c, s, _ in LENS_CASES])
def test_out_lens_edges(dev, monkeypatch, case, setting, tile):
    """MaskConv lengths beyond wo (masks nothing), at the column tile's edge (wo - 1 where one
    tile holds the row), 1, 0 and negative (an all-zero sample): columns >= len are exactly 0,
    the rest is within 1e-5 of float64."""
    set_env(monkeypatch, setting)
    cfg = with_n(CASES[case].cfg, 5)
    assert_rungs(cfg, (CASES[case].rungs[setting][0], None, None))
    r = ref64(cfg)
    ho, wo = out_hw(cfg)
    lens = [wo + 7, tile if wo > tile else wo - 1, 1, 0, -3]
    y, _, intact = run_fwd(cfg, Poisoned(r.x, dev), Poisoned(r.w, dev), Poisoned(r.b, dev), dev,
                           out_lens=lens)
    assert intact
    want = r.y.clone()
    for i, ln in enumerate(lens):
        cut = min(max(ln, 0), wo)
        want[i, :, :, cut:] = 0
        assert (y[i, :, :, cut:] == 0).all(), f"sample {i}: a column >= {ln} is not exactly 0"
    close(y, want, name=f"{case}-{setting} out_lens {lens}")


ZN_RUNGS = {("A", "default"): ("fwd_h3_2r", "dg_h3_2r", "wg_patch:2:1"),
            ("A", "x6"): ("fwd_x6_db", "dg_x6_q", "wg_patch:2:1"),
            ("B", "default"): ("fwd_h3_2r", "dg_h3_2r", "wg_h3_sw32"),
            ("B", "x6"): ("fwd_x6_db", "dg_x6_q", "wg_x6_sw")}


@pytest.mark.parametrize("setting", ["default", "x6"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_zero_and_nonfinite_samples(dev, monkeypatch, case, setting):
    """A fully masked utterance (an all-zero sample of x or dy) gives exactly the bias / exactly
    zero: the accumulators are 0 and the fp16x3 scale of a zero sample is a power of two.  An
    all-zero input channel of x and output channel of dy give exactly zero slices of dw.  A
    sample with a NaN and a +Inf leaves the other samples within 1e-5 of float64 (the fp16x3
    scale is per sample; padding selects, it does not multiply)."""
    set_env(monkeypatch, setting)
    cfg = with_n(CASES[case].cfg, 3)
    assert_rungs(cfg, ZN_RUNGS[case, setting])
    r = ref64(cfg)
    name = f"{case}-{setting}"
    w, b = Poisoned(r.w, dev), Poisoned(r.b, dev)

    for what in ("zero", "nonfinite"):
        x, dy = r.x.clone(), r.dy.clone()
        if what == "zero":
            x[1], dy[1] = 0, 0
        else:
            x[1, 0, 3, 2], x[1, -1, -1, -1] = float("nan"), float("inf")
            dy[1, 0, 3, 0], dy[1, -1, -1, -1] = float("nan"), float("inf")
        y, _, intact = run_fwd(cfg, Poisoned(x, dev), w, b, dev)
        assert intact
        dx, _, intact = run_dgrad(cfg, Poisoned(dy, dev), w, dev)
        assert intact
        for i in (0, 2):
            close(y[i], r.y[i], name=f"{name} {what} sample 1: y[{i}]")
            close(dx[i], r.dx[i], name=f"{name} {what} sample 1: dx[{i}]")
        if what == "zero":
            assert torch.equal(y[1], r.b.float()[:, None, None].expand_as(y[1])), "y[1] != bias"
            assert (dx[1] == 0).all(), "dx[1] != 0"

    x, dy = r.x.clone(), r.dy.clone()
    x[:, 1], dy[:, 2] = 0, 0
    want = r.dw.clone()
    want[2], want[:, 1] = 0, 0
    (dw, _), _, intact = run_wgrad(cfg, Poisoned(dy, dev), Poisoned(x, dev), dev, with_bias=False)
    assert intact
    assert (dw[2] == 0).all() and (dw[:, 1] == 0).all(), "dw of a zero channel is not exactly 0"
    close(dw, want, name=f"{name} zero channels: dw")


@pytest.mark.parametrize("case,setting", case_settings(STREAMING), ids=_ids(case_settings(STREAMING)))
def test_streaming_windows(dev, monkeypatch, case, setting):
    """The windows StreamingSession._conv_block feeds both convolutions (time padding 0, one
    and two output columns, out_lens = the full width), forward, in poison."""
    set_env(monkeypatch, setting)
    cfg, rungs = STREAMING[case]
    assert_rungs(cfg, rungs[setting])
    r = ref64(cfg)
    ho, wo = out_hw(cfg)
    assert wo in (1, 2)
    y, _, intact = run_fwd(cfg, Poisoned(r.x, dev), Poisoned(r.w, dev), Poisoned(r.b, dev), dev,
                           out_lens=[wo] * cfg[0])
    close(y, r.y, name=f"{case}-{setting} fwd {rungs[setting][0]}")
    assert intact


@pytest.mark.parametrize("case,setting", [("L1", "default"), ("L1", "fp32"), ("L2", "default")])
def test_dgrad_positions_without_a_tap(dev, monkeypatch, case, setting):
    """kh < sh leaves a stride class without taps, kw < sw columns without one: dx (pre-filled
    with NaN) is written there, as exact zeros."""
    set_env(monkeypatch, setting)
    cfg, rungs = CASES[case]
    assert_rungs(cfg, (None, rungs[setting][1], None))
    n, ci, h, w, co, kh, kw, sh, sw, ph, pw = cfg
    ho, wo = out_hw(cfg)
    r = ref64(cfg)
    dx, _, intact = run_dgrad(cfg, Poisoned(r.dy, dev), Poisoned(r.w, dev), dev)
    assert intact
    rows = torch.tensor([any((i + ph - k) % sh == 0 and 0 <= (i + ph - k) // sh < ho
                             for k in range(kh)) for i in range(h)])
    cols = torch.tensor([any((j + pw - k) % sw == 0 and 0 <= (j + pw - k) // sw < wo
                             for k in range(kw)) for j in range(w)])
    assert not rows.all(), "the shape has no row without a tap"
    assert (case == "L1") == bool(cols.all())
    assert (dx[:, :, ~rows, :] == 0).all(), "a row no tap reaches is not exactly 0"
    assert (dx[:, :, :, ~cols] == 0).all(), "a column no tap reaches is not exactly 0"
    close(dx, r.dx, name=f"{case}-{setting} dgrad {rungs[setting][1]}")


def test_argument_checks(dev, monkeypatch):
    """n == 0 is DS2_OK; a zero or negative size, a negative padding and ho or wo < 1 are
    DS2_INVALID_VALUE; all return before any launch (NULL pointers throughout).  A workspace
    one byte short of the plan's, or NULL, is DS2_WORKSPACE_TOO_SMALL and leaves the output
    untouched; a rung whose plan needs no workspace accepts NULL."""
    set_env(monkeypatch, "default")
    lib = _lib.load()
    good = (2, 4, 9, 20, 8, 3, 3, 2, 1, 1, 1)

    def fwd(d):
        return lib.ds2_conv2d_fwd(None, None, None, None, *d, None, None, 0, None)

    def dgrad(d):
        return lib.ds2_conv2d_dgrad(None, None, None, *d, None, 0, None)

    def wgrad(d):
        return lib.ds2_conv2d_wgrad(None, None, None, None, *d, None, 0, None)

    zero_n = (0,) + good[1:]
    assert fwd(zero_n) == OK and dgrad(zero_n) == OK and wgrad(zero_n) == OK
    bad = [good[:i] + (v,) + good[i + 1:] for i in range(1, 9) for v in (0, -1)]   # ci .. sw
    bad += [(-1,) + good[1:]]                                                      # n
    bad += [good[:9] + (-1, 1), good[:10] + (-1,)]                                 # ph, pw
    # ho, wo < 1: a kernel one row / column larger than the padded input, at strides 2 and 1
    bad += [(2, 4, 9, 20, 8, 12, 3, 2, 1, 1, 1), (2, 4, 9, 20, 8, 3, 23, 2, 2, 1, 1),
            (2, 4, 9, 20, 8, 12, 3, 1, 1, 1, 1), (2, 4, 9, 20, 8, 3, 23, 2, 1, 1, 1)]
    for d in bad:
        assert fwd(d) == INVALID_VALUE and dgrad(d) == INVALID_VALUE and wgrad(d) == INVALID_VALUE, d

    cfg, rungs = CASES["A"]
    p = assert_rungs(cfg, rungs["default"])
    assert all(p[d].ws_bytes > 0 for d in p)
    r = ref64(cfg)
    n, ci, h, w, co, kh, kw = cfg[:7]
    x, wt, dy = Poisoned(r.x, dev), Poisoned(r.w, dev), Poisoned(r.dy, dev)
    y, dx, dw = Poisoned(r.y.shape, dev), Poisoned(r.x.shape, dev), Poisoned(r.w.shape, dev)
    for short in (True, False):      # one byte short; no workspace at all
        ws = {d: Workspace(p[d].ws_bytes, dev) for d in p}
        arg = {d: (ws[d].ptr, p[d].ws_bytes - 1) if short else (None, p[d].ws_bytes) for d in p}
        assert lib.ds2_conv2d_fwd(x.ptr, wt.ptr, None, y.ptr, *cfg, None, *arg["fwd"],
                                  None) == WORKSPACE_TOO_SMALL
        assert lib.ds2_conv2d_dgrad(dy.ptr, wt.ptr, dx.ptr, *cfg, *arg["dgrad"],
                                    None) == WORKSPACE_TOO_SMALL
        assert lib.ds2_conv2d_wgrad(dy.ptr, x.ptr, dw.ptr, None, *cfg, *arg["wgrad"],
                                    None) == WORKSPACE_TOO_SMALL
        torch.cuda.synchronize()
        for out in (y, dx, dw):
            assert torch.isnan(out.read()).all() and out.intact()
        assert all(ws[d].intact() for d in p)

    for case in ("J2", "H"):         # fwd_c1, fwd_gemm: no workspace in the plan
        cfg, rungs = CASES[case]
        assert assert_rungs(cfg, rungs["default"])["fwd"].ws_bytes == 0
        r = ref64(cfg)
        x, wt, y = Poisoned(r.x, dev), Poisoned(r.w, dev), Poisoned(r.y.shape, dev)
        st = lib.ds2_conv2d_fwd(x.ptr, wt.ptr, None, y.ptr, *cfg, None, None, 0, None)
        assert st == OK
        torch.cuda.synchronize()
        close(y.read(), r.y - r.b[:, None, None], name=f"{case} fwd without a workspace")


@pytest.mark.parametrize("case,setting", case_settings({k: CASES[k] for k in ("A", "G")}),
                         ids=_ids(case_settings({k: CASES[k] for k in ("A", "G")})))
def test_rung_in_poison_four_byte_aligned(dev, monkeypatch, case, setting):
    """include/ds2hip.h: Conv2d operands need 4-byte alignment only.  test_rung_in_poison with
    x, w, bias, dy, y, dx, dw and dbias at addresses that are 4-byte aligned and no more.

    Decided from the code before it was run: every kernel of conv.hip and conv_split.hip reads
    the caller's x / dy through 4-byte buffer loads (conv_rsrc) or plain float loads, w and
    bias through plain float loads, and writes y / dx / dw / dbias one float at a time; the
    16-byte buffer loads and vector LDS stores all address the weight images inside the
    workspace (256-byte aligned, offsets multiples of 16); conv_h3_samax_kernel takes its
    float4 loads only where the sample's chunk starts 16-byte aligned and strides by floats
    otherwise."""
    set_env(monkeypatch, setting)
    cfg, rungs = CASES[case]
    assert_rungs(cfg, rungs[setting])
    _run_all(cfg, rungs[setting], dev, f"{case}-{setting} 4-byte", lead=LEAD4)
