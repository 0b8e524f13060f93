"""GPU: the Conv1d kernels and the Wav2Letter pointwise kernels (csrc/conv1d.hip) against
float64 across the calling contract of ds2_conv1d_fwd[_amax] / _dgrad / _wgrad[_amax]: every
path of the dispatch at its tile, channel-chunk, stage-count, slab and padding edges
(conv1d_common.CASES; test_conv1d_contract_cpu.py proves from the library's plan that the table
reaches them), operands inside poisoned allocations, a workspace of exactly the query's (or the
plan's) size that held 0xFF with canaries around it, exact values where every term is a zero,
zero and non-finite rows under the window scale, caller-supplied maxima, the status codes,
empty batches, operands that are 4-byte aligned only, and the grid-stride kernels in their
second iteration.

Two bounds on every result (conv1d_common.close, printed with pytest -s): the project's
max |err| <= 1e-5 max |ref|, and |err| <= 2e-6 (|w| conv |x| + |b|) elementwise, 8 x what float32
torch on the CPU needs on these shapes."""
import pytest
import torch

from ds2amd import _lib, ops

from conv1d_common import (CASES, GEMM, LEAD4, LEAD16, SCALAR, SETTINGS, VEC, Poisoned, Workspace,
                           assert_paths, case_settings, close, nct, out_len, query, ref64, run_dgrad,
                           run_fwd, run_wgrad, set_env, tnc, want_paths, with_n)
from conv_common import WS_LEAD

pytestmark = pytest.mark.gpu

OK, INVALID_VALUE, UNSUPPORTED_SHAPE, WORKSPACE_TOO_SMALL = 0, 1, 2, 5


def _ids(pairs):
    return [f"{c}-{s}" for c, s in pairs]


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _operands(r, dev, lead=LEAD16):
    return (Poisoned(tnc(r.x), dev, lead), Poisoned(r.w, dev, lead), Poisoned(r.b, dev, lead),
            Poisoned(tnc(r.dy), dev, lead))


def _run_all(cfg, want, dev, name, lead=LEAD16):
    """Forward with bias, dgrad and wgrad with dbias in poison against ref64(cfg), each a second
    time on a workspace that held zeros where the first held 0xFF: the same bits."""
    r = ref64(cfg)
    x, w, b, dy = _operands(r, dev, lead)
    y, pf, intact = run_fwd(cfg, x, w, b, dev, lead=lead)
    close(y, r.y, r.y_mag, f"{name} fwd {pf.path}", r.cpu32["y"])
    assert intact, f"{name}: a write outside y or outside the forward workspace"
    dx, pd, intact = run_dgrad(cfg, dy, w, dev, lead=lead)
    close(dx, r.dx, r.dx_mag, f"{name} dgrad {pd.path}", r.cpu32["dx"])
    assert intact, f"{name}: a write outside dx or outside the dgrad workspace"
    (dw, db), pw, intact = run_wgrad(cfg, dy, x, dev, lead=lead)
    close(dw, r.dw, r.dw_mag, f"{name} wgrad {pw.path}", r.cpu32["dw"])
    close(db, r.db, r.db_mag, f"{name} dbias", r.cpu32["db"])
    assert intact, f"{name}: a write outside dw / dbias or outside the wgrad workspace"
    assert (pf.path, pd.path, pw.path) == tuple(want), (name, pf.path, pd.path, pw.path)
    # stale maxima (0xFFFFFFFF is what atomicMax cannot exceed), NaN in the padded weight
    # channels, slabs not fully written
    y0, _, intact = run_fwd(cfg, x, w, b, dev, lead=lead, ws_fill=0x00)
    assert intact and _bits(y, y0), f"{name}: y depends on what the workspace held"
    dx0, _, intact = run_dgrad(cfg, dy, w, dev, lead=lead, ws_fill=0x00)
    assert intact and _bits(dx, dx0), f"{name}: dx depends on what the workspace held"
    (dw0, db0), _, intact = run_wgrad(cfg, dy, x, dev, lead=lead, ws_fill=0x00)
    assert intact and _bits(dw, dw0) and _bits(db, db0), f"{name}: dw depends on what the workspace held"


@pytest.mark.parametrize("case,setting", case_settings(), ids=_ids(case_settings()))
def test_path_in_poison(dev, monkeypatch, case, setting):
    """Each case on operands surrounded by NaN, outputs pre-filled with NaN and surrounded by
    canaries, a 0xFF-filled workspace of exactly the query's bytes with canaries around it."""
    set_env(monkeypatch, setting)
    cfg = CASES[case].cfg
    want = want_paths(case, setting)
    assert_paths(cfg, want, addr=4 * LEAD16)
    _run_all(cfg, want, dev, f"{case}-{setting}")


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", ["F2", "H"])
def test_rows_that_see_only_padding_are_exactly_the_bias(dev, monkeypatch, case, setting):
    set_env(monkeypatch, setting)
    cfg = CASES[case].cfg
    t, n, ci, co, k, s, p = cfg
    r = ref64(cfg)
    x, w, b, _ = _operands(r, dev)
    y, _, intact = run_fwd(cfg, x, w, b, dev)
    assert intact
    rows = [to for to in range(out_len(cfg)) if all(not 0 <= to * s - p + j < t for j in range(k))]
    assert rows == {"F2": [0, 22], "H": [0, 1, 13, 14]}[case]
    want = r.b.float()[None, :, None].expand(n, co, len(rows))
    assert torch.equal(y[:, :, rows], want), "a row of padding only is not exactly the bias"


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", ["F1", "G"])
def test_dgrad_rows_without_a_tap_are_exactly_zero(dev, monkeypatch, case, setting):
    """s > k (or k = 1 at s = 2) and (T + 2p - k) % s != 0 leave input rows no tap reaches: dx
    (pre-filled with NaN) is written there, as exact zeros."""
    set_env(monkeypatch, setting)
    cfg = CASES[case].cfg
    t, n, ci, co, k, s, p = cfg
    r = ref64(cfg)
    _, w, _, dy = _operands(r, dev)
    dx, _, intact = run_dgrad(cfg, dy, w, dev)
    assert intact
    hit = torch.tensor([any((ti + p - j) % s == 0 and 0 <= (ti + p - j) // s < out_len(cfg)
                            for j in range(k)) for ti in range(t)])
    assert int((~hit).sum()) == {"F1": 10, "G": 14}[case]
    assert (dx[:, :, ~hit] == 0).all(), "a row no tap reaches is not exactly 0"
    close(dx, r.dx, r.dx_mag, f"{case}-{setting} dgrad")


@pytest.mark.parametrize("case,setting", case_settings(["A", "B", "I", "P1"]),
                         ids=_ids(case_settings(["A", "B", "I", "P1"])))
def test_path_in_poison_four_byte_aligned(dev, monkeypatch, case, setting):
    """include/ds2hip.h: Conv1d operands need 4-byte alignment only.  test_path_in_poison with x,
    w, bias, dy, y, dx, dw and dbias at addresses that are 4-byte aligned and no more.

    Decided from the code before it was run.  c1_igemm_kernel<true> is the only kernel that
    reads a caller's array (x, or dy in dgrad) with 16-byte loads, and c1_plan selects it only
    where that address is 16-byte aligned and the channel count a multiple of 4 (every row then
    starts 16-byte aligned and a float4 never straddles the channel edge); otherwise
    c1_igemm_kernel<false> loads single floats.  Its other 16-byte loads read the re-laid
    weights in the workspace (256-byte aligned sections, rows of k pad32(C) floats).
    c1_relayout_w_kernel, c1_rowmax_kernel, c1_colmax_kernel, c1_wgrad_kernel,
    c1_wgrad_reduce_kernel and c1_general_kernel read and write single floats; y / dx / dw are
    stored one float at a time.  ds2_colsum (dbias) and ds2_sgemm_ws (k = 1) choose their
    16-byte forms by the addresses they are given."""
    set_env(monkeypatch, setting)
    cfg = CASES[case].cfg
    want = want_paths(case, setting)
    if setting == "default" and cfg[2] % 4 == 0 and want[0] in (VEC, SCALAR):
        want = (SCALAR,) + tuple(want[1:])
    if setting == "default" and cfg[3] % 4 == 0 and want[1] in (VEC, SCALAR):
        want = (want[0], SCALAR, want[2])
    if setting == "default":
        assert {"A": SCALAR, "B": SCALAR, "I": SCALAR, "P1": GEMM}[case] == want[0]
    assert_paths(cfg, want, addr=4 * LEAD4)
    _run_all(cfg, want, dev, f"{case}-{setting} 4-byte", lead=LEAD4)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", ["B", "I"])
def test_zero_samples_and_channels(dev, monkeypatch, case, setting):
    """An all-zero sample of x / dy gives exactly the bias / exactly 0 (the accumulators are 0
    and the scale of an all-zero window is a power of two), an all-zero output channel of w
    exactly the bias, an all-zero input channel of x and output channel of dy exactly-zero
    slices of dw; everything else stays within both bounds."""
    set_env(monkeypatch, setting)
    cfg = with_n(CASES[case].cfg, 3)
    assert_paths(cfg, want_paths(case, setting), addr=4 * LEAD16)
    t, n, ci, co, k, s, p = cfg
    r = ref64(cfg)
    name = f"{case}-{setting}"
    _, w, b, _ = _operands(r, dev)

    x, dy = r.x.clone(), r.dy.clone()
    x[1], dy[1] = 0, 0
    y, _, intact = run_fwd(cfg, Poisoned(tnc(x), dev), w, b, dev)
    assert intact
    dx, _, intact = run_dgrad(cfg, Poisoned(tnc(dy), dev), w, dev)
    assert intact
    for i in (0, 2):
        close(y[i], r.y[i], r.y_mag[i], f"{name} zero sample 1: y[{i}]")
        close(dx[i], r.dx[i], r.dx_mag[i], f"{name} zero sample 1: dx[{i}]")
    assert torch.equal(y[1], r.b.float()[:, None].expand_as(y[1])), "y[1] != bias"
    assert (dx[1] == 0).all(), "dx[1] != 0"

    wz = r.w.clone()
    wz[5] = 0
    y, _, intact = run_fwd(cfg, Poisoned(tnc(r.x), dev), Poisoned(wz, dev), b, dev)
    assert intact
    assert (y[:, 5] == r.b[5].float()).all(), "a zero output channel of w does not give the bias"
    keep = [c for c in range(co) if c != 5]
    close(y[:, keep], r.y[:, keep], r.y_mag[:, keep], f"{name} zero channel of w: the others")

    x, dy = r.x.clone(), r.dy.clone()
    x[:, 1], dy[:, 2] = 0, 0
    want, mag = r.dw.clone(), r.dw_mag.clone()
    want[2], want[:, 1], mag[2], mag[:, 1] = 0, 0, 0, 0
    (dw, _), _, intact = run_wgrad(cfg, Poisoned(tnc(dy), dev), Poisoned(tnc(x), dev), dev,
                                   with_bias=False)
    assert intact
    close(dw, want, mag, f"{name} zero channels: dw")       # asserts exact zeros where mag == 0
    assert (dw[2] == 0).all() and (dw[:, 1] == 0).all()


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", ["B", "I"])
def test_nonfinite_rows(dev, monkeypatch, case, setting):
    """A NaN and a +Inf in one time row t0 of sample 1 (x for the forward, dy for dgrad): the
    scale of a window is the maximum of its rows' maxima, c1_rowmax_kernel's fmaxf skips the NaN
    and h3_exp maps the Inf to exponent 0, so every output row whose window holds t0 must come
    out non-finite (none quietly finite), every other row of sample 1 and the other samples
    within both bounds.  A +Inf in one input channel of x (wgrad): that channel's dw is not all
    finite, every other channel's is within both bounds."""
    set_env(monkeypatch, setting)
    cfg = with_n(CASES[case].cfg, 3)
    assert_paths(cfg, want_paths(case, setting), addr=4 * LEAD16)
    t, n, ci, co, k, s, p = cfg
    assert s == 1
    to_n = out_len(cfg)
    r = ref64(cfg)
    name = f"{case}-{setting}"
    _, w, b, _ = _operands(r, dev)
    t0 = 17

    x = r.x.clone()
    x[1, 3, t0], x[1, ci - 1, t0] = float("nan"), float("inf")
    y, _, intact = run_fwd(cfg, Poisoned(tnc(x), dev), w, b, dev)
    assert intact
    hit = torch.tensor([to - p <= t0 <= to - p + k - 1 for to in range(to_n)])
    assert 0 < int(hit.sum()) == k < to_n
    assert not torch.isfinite(y[1][:, hit]).any(), "a window that holds the NaN / Inf row is finite"
    close(y[1][:, ~hit], r.y[1][:, ~hit], r.y_mag[1][:, ~hit], f"{name} nonfinite x: y[1], other rows")
    for i in (0, 2):
        close(y[i], r.y[i], r.y_mag[i], f"{name} nonfinite x: y[{i}]")

    dy = r.dy.clone()
    dy[1, 3, t0], dy[1, co - 1, t0] = float("nan"), float("inf")
    dx, _, intact = run_dgrad(cfg, Poisoned(tnc(dy), dev), w, dev)
    assert intact
    hit = torch.tensor([0 <= ti + p - t0 <= k - 1 for ti in range(t)])
    assert 0 < int(hit.sum()) == k < t
    assert not torch.isfinite(dx[1][:, hit]).any(), "a dx row that reads the NaN / Inf row is finite"
    close(dx[1][:, ~hit], r.dx[1][:, ~hit], r.dx_mag[1][:, ~hit], f"{name} nonfinite dy: dx[1], other rows")
    for i in (0, 2):
        close(dx[i], r.dx[i], r.dx_mag[i], f"{name} nonfinite dy: dx[{i}]")

    x = r.x.clone()
    x[1, 7, t0] = float("inf")
    (dw, _), _, intact = run_wgrad(cfg, Poisoned(tnc(r.dy), dev), Poisoned(tnc(x), dev), dev,
                                   with_bias=False)
    assert intact
    keep = [c for c in range(ci) if c != 7]
    assert not torch.isfinite(dw[:, 7]).all(), "dw of the channel that holds the Inf is finite"
    close(dw[:, keep], r.dw[:, keep], r.dw_mag[:, keep], f"{name} Inf in channel 7 of x: the other channels")


@pytest.mark.parametrize("case", ["B", "I"])
def test_caller_supplied_maxima(dev, monkeypatch, case):
    """ds2_conv1d_fwd_amax / ds2_conv1d_wgrad_amax: exact maxima give the bits of the call that
    computes them itself and save one pass; maxima four times too large (include/ds2hip.h: "an
    upper bound is valid") stay within both bounds; DS2_CONV1D=0 ignores them."""
    cfg = CASES[case].cfg
    r = ref64(cfg)
    x, w, b, dy = _operands(r, dev)
    xd = tnc(r.x).float().to(dev)
    rmax, cmax = xd.abs().amax(2).reshape(-1).contiguous(), xd.abs().amax((0, 1)).contiguous()
    exact = {"fwd": rmax.view(torch.int32), "wgrad": cmax.view(torch.int32)}
    loose = {"fwd": (rmax * 4).view(torch.int32), "wgrad": (cmax * 4).view(torch.int32)}
    assert torch.equal(loose["fwd"] - exact["fwd"], torch.full_like(exact["fwd"], 2 << 23))

    for setting in SETTINGS:
        set_env(monkeypatch, setting)
        y, pl, _ = run_fwd(cfg, x, w, b, dev)
        (dw, db), pw, _ = run_wgrad(cfg, dy, x, dev)
        for kind, am in (("exact", exact), ("loose", loose)):
            ya, pla, intact = run_fwd(cfg, x, w, b, dev, amax=am["fwd"].data_ptr())
            assert intact
            (dwa, dba), pwa, intact = run_wgrad(cfg, dy, x, dev, amax=am["wgrad"].data_ptr())
            assert intact
            if setting == "default":
                assert (pl.amax_passes, pla.amax_passes, pw.amax_passes, pwa.amax_passes) == (2, 1, 2, 1)
            else:
                assert (pl.amax_passes, pla.amax_passes, pw.amax_passes, pwa.amax_passes) == (0, 0, 0, 0)
            if kind == "exact" or setting == "general":
                assert _bits(y, ya), f"{case}-{setting} {kind} row maxima change y"
                assert _bits(dw, dwa), f"{case}-{setting} {kind} column maxima change dw"
            else:
                close(ya, r.y, r.y_mag, f"{case} fwd, row maxima x 4")
                close(dwa, r.dw, r.dw_mag, f"{case} wgrad, column maxima x 4")
            assert _bits(db, dba)


def test_an_edit_in_place_drops_the_tagged_maxima(dev, monkeypatch):
    """BNReLUFn leaves its output's maxima for the Conv1d that reads it next; y.detach().mul_()
    changes the values behind them.  The convolution must then compute its own: maxima 1000
    times too small would overflow the fp16 split.  Finite, and the bits of the same values in
    a fresh tensor, forward and weight gradient."""
    set_env(monkeypatch, "default")
    t, n, c, co = 23, 3, 32, 48
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(t * n, c, generator=g) * 3 + 1).to(dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    w = (torch.randn(co, c, 13, generator=g) * 0.1).to(dev)
    dy = torch.randn(t, n, co, generator=g).to(dev)
    y = ops.BNReLUFn.apply(x, gamma, beta, rm, rv, True, 0.1, 1e-5)
    assert any(e[1] == y.data_ptr() for e in ops._OPERAND_AMAX), "the shape no longer tags its maxima"
    y.detach().mul_(1000.0)
    outs = []
    for src in (y.view(t, n, c), y.clone().view(t, n, c)):
        wt = w.clone().requires_grad_(True)
        out = ops.Conv1dFn.apply(src, wt, None, 1, 6)
        out.backward(dy)
        outs.append((out.detach(), wt.grad))
    for a, b_ in zip(*outs):
        assert torch.isfinite(a).all() and _bits(a, b_)


def test_status_codes_and_the_planned_workspace(dev, monkeypatch):
    """B on the fast path, every direction: NULL or one byte fewer than the plan's bytes is
    DS2_WORKSPACE_TOO_SMALL with the outputs untouched; exactly the plan's bytes (less than the
    query's) is correct with every canary intact, so the kernels stay inside what the check
    demands.  A path whose plan says 0 takes NULL."""
    lib = _lib.load()
    set_env(monkeypatch, "default")
    cfg = CASES["B"].cfg
    t, n, ci, co, k, s, p = cfg
    r = ref64(cfg)
    x, w, b, dy = _operands(r, dev)
    pl = assert_paths(cfg, CASES["B"].paths, addr=4 * LEAD16)
    assert all(0 < pl[d].ws_bytes <= query(d, cfg) for d in pl)
    y, dx = Poisoned((out_len(cfg), n, co), dev), Poisoned((t, n, ci), dev)
    dw, db = Poisoned((co, ci, k), dev), Poisoned((co,), dev)
    for short in (True, False):      # one byte short; no workspace at all
        ws = {d: Workspace(pl[d].ws_bytes, dev) for d in pl}
        arg = {d: (ws[d].ptr, pl[d].ws_bytes - 1) if short else (None, pl[d].ws_bytes) for d in pl}
        assert lib.ds2_conv1d_fwd(x.ptr, w.ptr, b.ptr, y.ptr, *cfg, *arg["fwd"], None) == WORKSPACE_TOO_SMALL
        assert lib.ds2_conv1d_dgrad(dy.ptr, w.ptr, dx.ptr, *cfg, *arg["dgrad"], None) == WORKSPACE_TOO_SMALL
        assert lib.ds2_conv1d_wgrad(dy.ptr, x.ptr, dw.ptr, db.ptr, *cfg, *arg["wgrad"],
                                    None) == WORKSPACE_TOO_SMALL
        torch.cuda.synchronize()
        for out in (y, dx, dw, db):
            assert torch.isnan(out.read()).all() and out.intact()
        assert all(ws[d].intact() for d in pl)

    yy, _, intact = run_fwd(cfg, x, w, b, dev, ws_bytes=pl["fwd"].ws_bytes)
    close(yy, r.y, r.y_mag, "B fwd on the plan's bytes")
    assert intact
    dd, _, intact = run_dgrad(cfg, dy, w, dev, ws_bytes=pl["dgrad"].ws_bytes)
    close(dd, r.dx, r.dx_mag, "B dgrad on the plan's bytes")
    assert intact
    (ww, bb), _, intact = run_wgrad(cfg, dy, x, dev, ws_bytes=pl["wgrad"].ws_bytes)
    close(ww, r.dw, r.dw_mag, "B wgrad on the plan's bytes")
    close(bb, r.db, r.db_mag, "B dbias on the plan's bytes")
    assert intact

    # no workspace in the plan: the general kernels, and the k = 1 GEMM (ds2_sgemm_ws)
    for case, setting in (("B", "general"), ("D1", "default"), ("P1", "default")):
        set_env(monkeypatch, setting)
        cfg = CASES[case].cfg
        t, n, ci, co, k, s, p = cfg
        pl = assert_paths(cfg, want_paths(case, setting), addr=4 * LEAD16)
        assert pl["fwd"].ws_bytes == 0 and pl["dgrad"].ws_bytes == 0 and pl["wgrad"].ws_bytes > 0
        r = ref64(cfg)
        x, w, b, dy = _operands(r, dev)
        y, dx = Poisoned((out_len(cfg), n, co), dev), Poisoned((t, n, ci), dev)
        assert lib.ds2_conv1d_fwd(x.ptr, w.ptr, b.ptr, y.ptr, *cfg, None, 0, None) == OK
        assert lib.ds2_conv1d_dgrad(dy.ptr, w.ptr, dx.ptr, *cfg, None, 0, None) == OK
        torch.cuda.synchronize()
        close(nct(y.read()), r.y, r.y_mag, f"{case}-{setting} fwd without a workspace")
        close(nct(dx.read()), r.dx, r.dx_mag, f"{case}-{setting} dgrad without a workspace")
        assert y.intact() and dx.intact()


def test_empty_batches(dev, monkeypatch):
    """t == 0 and n == 0: ds2_conv1d_wgrad overwrites dw and dbias with the empty sum (exact
    zeros) without a workspace; forward and dgrad return DS2_OK and write nothing."""
    lib = _lib.load()
    for setting in SETTINGS:
        set_env(monkeypatch, setting)
        for cfg in ((0, 2, 20, 24, 3, 1, 1), (9, 0, 20, 24, 3, 1, 1), (0, 2, 20, 24, 1, 1, 0)):
            t, n, ci, co, k, s, p = cfg
            dw, db = Poisoned((co, ci, k), dev), Poisoned((co,), dev)
            assert lib.ds2_conv1d_wgrad(None, None, dw.ptr, db.ptr, *cfg, None, 0, None) == OK
            y, dx = Poisoned((5, 2, co), dev), Poisoned((5, 2, ci), dev)
            assert lib.ds2_conv1d_fwd(None, None, None, y.ptr, *cfg, None, 0, None) == OK
            assert lib.ds2_conv1d_dgrad(None, None, dx.ptr, *cfg, None, 0, None) == OK
            torch.cuda.synchronize()
            assert (dw.read() == 0).all() and (db.read() == 0).all() and dw.intact() and db.intact()
            assert torch.isnan(y.read()).all() and torch.isnan(dx.read()).all()
            assert y.intact() and dx.intact()


@pytest.mark.parametrize("case,setting", case_settings(["I", "R"]), ids=_ids(case_settings(["I", "R"])))
def test_two_runs_give_the_same_bits(dev, monkeypatch, case, setting):
    set_env(monkeypatch, setting)
    cfg = CASES[case].cfg
    x, w, b, dy = _operands(ref64(cfg), dev)
    a = (run_fwd(cfg, x, w, b, dev)[0], run_dgrad(cfg, dy, w, dev)[0], *run_wgrad(cfg, dy, x, dev)[0])
    c = (run_fwd(cfg, x, w, b, dev)[0], run_dgrad(cfg, dy, w, dev)[0], *run_wgrad(cfg, dy, x, dev)[0])
    assert all(_bits(u, v) for u, v in zip(a, c))


# ---------------------------------------------------------------------------
# pointwise kernels

U = 2.0 ** -24      # float32 unit roundoff


FLT_MIN = 2.0 ** -126


def _within(got, ref, mag, rel, name):
    """|got - ref| <= rel * mag + FLT_MIN elementwise (a result below float32's normal range may
    be flushed to zero); prints the worst ratio to the bound."""
    got, ref, mag = got.double().cpu(), ref.double(), mag.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    ratio = (got - ref).abs() / (rel * mag + FLT_MIN)
    print(f"CONV1D_CONTRACT {name}: componentwise err / bound = {ratio.max().item():.3f}")
    assert ratio.max().item() <= 1, f"{name}: {ratio.max().item():.3f} x the bound {rel:.1e} * magnitude"


def _rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()


def _glu(dev, x, dy, name):
    """ds2_glu_fwd / ds2_glu_bwd on Poisoned operands.  sigmoid = 1 / (1 + expf(-b)): expf and
    the division are within 2 and 2.5 units in the last place, the sum and each product within
    0.5, so y = a sg is within 6 u |y| and dx_a = g sg within 6 u |dx_a|; (1 - sg) carries sg's
    absolute error, so dx_b = g a sg (1 - sg) is within 8 u |g a sg|.  Asserted: 16 u ~ 1e-6."""
    rows, c2 = x.shape
    c = c2 // 2
    a, bgate = x[:, :c], x[:, c:]
    sg = torch.sigmoid(bgate)
    xp, dyp = Poisoned(x, dev), Poisoned(dy, dev)
    y, dx = Poisoned((rows, c), dev), Poisoned((rows, c2), dev)
    lib = _lib.load()
    assert lib.ds2_glu_fwd(xp.ptr, rows, c, y.ptr, None) == OK
    assert lib.ds2_glu_bwd(dyp.ptr, xp.ptr, rows, c, dx.ptr, None) == OK
    torch.cuda.synchronize()
    assert y.intact() and dx.intact(), f"{name}: a write outside y or dx"
    yv, dxv = y.read(), dx.read()
    _within(yv, a * sg, (a * sg).abs(), 16 * U, f"{name} y")
    _within(dxv[:, :c], dy * sg, (dy * sg).abs(), 16 * U, f"{name} dx_a")
    _within(dxv[:, c:], dy * a * sg * (1 - sg), (dy * a * sg).abs(), 16 * U, f"{name} dx_b")
    return yv, dxv


@pytest.mark.parametrize("rows,c", [(57, 1), (57, 25), (57, 64), (2049, 1024)])
def test_glu_in_poison(dev, rows, c):
    """(2049, 1024): 2 098 176 outputs, the second iteration of the grid-stride loops."""
    g = torch.Generator().manual_seed(1000 * rows + c)
    _glu(dev, _rnd(g, rows, 2 * c) * 2, _rnd(g, rows, c), f"glu {rows}x{c}")


def test_glu_saturated_gates(dev):
    """Gates at +-100 and +-1e4 (expf overflows to inf at -b > 88.7): finite, y = a or 0 to
    1e-6, and the gate gradient exactly 0."""
    g = torch.Generator().manual_seed(3)
    rows, c = 8, 25
    x = _rnd(g, rows, 2 * c)
    gates = torch.tensor([100.0, -100.0, 1e4, -1e4], dtype=torch.float64)
    x[:, c:] = gates.repeat(rows * c // 4 + 1)[:rows * c].view(rows, c)
    dy = _rnd(g, rows, c)
    y, dx = _glu(dev, x, dy, "glu saturated")
    on = x[:, c:] > 0
    a = x[:, :c]
    assert ((y.double() - torch.where(on, a, torch.zeros_like(a))).abs() <= 1e-6 * a.abs()).all()
    assert (dx[:, c:] == 0).all(), "the gradient of a saturated gate is not exactly 0"


def _bn_args(g, c):
    mean, invstd = _rnd(g, c), (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).float().double()
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).float().double()
    return mean, invstd, gamma, _rnd(g, c)


def _bn_ref(x, mean, invstd, gamma, beta):
    """v = gamma ((x - mean) invstd) + beta in float64 and its magnitude |gamma| (|x| + |mean|)
    invstd + |beta|: the subtraction, the two products and the sum round once each, every
    rounding at most u times a result the magnitude bounds: |v32 - v| <= 4 u mag + O(u^2) (an
    FMA contraction only lowers it).  Asserted: 5 u mag."""
    v = gamma * ((x - mean) * invstd) + beta
    return v, gamma.abs() * (x.abs() + mean.abs()) * invstd + beta.abs()


@pytest.mark.parametrize("rows,c,lead,form", [(4100, 2048, LEAD16, "float4"), (2049, 1025, LEAD16, "scalar"),
                                              (57, 64, LEAD4, "scalar by address"), (57, 64, LEAD16, "float4")])
def test_bn_relu_apply_in_poison(dev, rows, c, lead, form):
    """4100 x 2048 / 4 and 2049 x 1025 elements: the second grid-stride iteration of the float4
    and the scalar form.  The ReLU pattern equals float64's wherever the pre-activation is
    farther from 0 than 1e-5 of the largest."""
    g = torch.Generator().manual_seed(rows + c)
    x = _rnd(g, rows, c) * 3 + 1
    x = x.float().double()
    mean, invstd, gamma, beta = _bn_args(g, c)
    v, mag = _bn_ref(x, mean, invstd, gamma, beta)
    ops_ = [Poisoned(a, dev, lead) for a in (x, mean, invstd, gamma, beta)]
    y = Poisoned((rows, c), dev, lead)
    st = _lib.load().ds2_bn_relu_apply(ops_[0].ptr, rows, c, *(o.ptr for o in ops_[1:]), y.ptr, None)
    assert st == OK
    torch.cuda.synchronize()
    assert y.intact(), "a write outside y"
    got = y.read()
    _within(got, v.clamp_min(0), mag, 5 * U, f"bn_relu_apply {rows}x{c} {form}")
    clear = v.abs() > 1e-5 * v.abs().max()
    assert torch.equal((got > 0)[clear], (v > 0)[clear]), "the ReLU pattern differs from float64's"


def test_bn_relu_bwd_masks_every_element(dev):
    """2049 x 1025: relu_mask_kernel's second grid-stride iteration.  dz, which the call leaves
    at the head of its workspace, is dy where y > 0 and 0 elsewhere, bit for bit; dx, dgamma
    and dbeta (ds2_bn_backward on that dz, covered at its own edges by test_gpu_bn_contract.py)
    are within the project's 1e-5 of max |ref| of the float64 formula."""
    rows, c = 2049, 1025
    g = torch.Generator().manual_seed(77)
    x = (_rnd(g, rows, c) * 3 + 1).float().double()
    _, _, gamma, beta = _bn_args(g, c)
    mean = x.mean(0).float().double()           # the batch statistics, as float32 stores them
    invstd = (x.var(0, unbiased=False) + 1e-5).rsqrt().float().double()
    v, _ = _bn_ref(x, mean, invstd, gamma, beta)
    yv = v.clamp_min(0).float().double()
    dy = _rnd(g, rows, c)
    dz = torch.where(yv > 0, dy, torch.zeros_like(dy))
    xhat = (x - mean) * invstd
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dxr = gamma * invstd * (dz - dbeta / rows - xhat * dgamma / rows)
    ins = [Poisoned(a, dev) for a in (dy, yv, x, mean, invstd, gamma, beta)]
    dx, dg, dbt = Poisoned((rows, c), dev), Poisoned((c,), dev), Poisoned((c,), dev)
    nbytes = _lib.size("ds2_bn_relu_bwd_workspace_size", rows, c)
    ws = Workspace(nbytes, dev)
    lib = _lib.load()
    st = lib.ds2_bn_relu_bwd(ins[0].ptr, ins[1].ptr, ins[2].ptr, rows, c, *(o.ptr for o in ins[3:]),
                             dx.ptr, dg.ptr, dbt.ptr, ws.ptr, nbytes, None)
    _lib.check(st, "ds2_bn_relu_bwd")
    torch.cuda.synchronize()
    assert dx.intact() and dg.intact() and dbt.intact() and ws.intact()
    dz_dev = ws.buf[WS_LEAD:WS_LEAD + 4 * rows * c].view(torch.float32).view(rows, c).cpu()
    assert _bits(dz_dev, dz.float()), "dz is not dy masked by y > 0"
    for got, ref, nm in ((dx, dxr, "dx"), (dg, dgamma, "dgamma"), (dbt, dbeta, "dbeta")):
        err = (got.read().double() - ref).abs().max().item()
        print(f"CONV1D_CONTRACT bn_relu_bwd {nm}: err / bound = {err / (1e-5 * ref.abs().max().item()):.3f}")
        assert err <= 1e-5 * ref.abs().max().item(), nm
    assert lib.ds2_bn_relu_bwd(ins[0].ptr, ins[1].ptr, ins[2].ptr, rows, c, *(o.ptr for o in ins[3:]),
                               dx.ptr, dg.ptr, dbt.ptr, ws.ptr, nbytes - 1, None) == WORKSPACE_TOO_SMALL


def test_bn_relu_apply_amax_contract(dev):
    """c = 2048 (the widest) is accepted: y equals ds2_bn_relu_apply's bits and the maxima are
    those of the stored y.  c = 2052, c = 30, an operand that is 4-byte aligned only and NULL
    maxima return DS2_UNSUPPORTED_SHAPE (3 x) and DS2_INVALID_VALUE with nothing written."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)

    def call(rows, c, lead_x=LEAD16, null=False):
        x = (_rnd(g, rows, c) * 3 + 1).float().double()
        args = _bn_args(g, c)
        xp = Poisoned(x, dev, lead_x)
        ap = [Poisoned(a, dev) for a in args]
        y, rmax, cmax = Poisoned((rows, c), dev), Poisoned((rows,), dev), Poisoned((c,), dev)
        st = lib.ds2_bn_relu_apply_amax(xp.ptr, rows, c, *(o.ptr for o in ap), y.ptr,
                                        None if null else rmax.ptr, None if null else cmax.ptr, None)
        y2 = Poisoned((rows, c), dev)
        assert lib.ds2_bn_relu_apply(xp.ptr, rows, c, *(o.ptr for o in ap), y2.ptr, None) == OK
        torch.cuda.synchronize()
        assert y.intact() and rmax.intact() and cmax.intact()
        return st, y.read(), rmax.read(), cmax.read(), y2.read()

    st, y, rmax, cmax, y2 = call(70, 2048)
    assert st == OK and _bits(y, y2)
    assert _bits(rmax, y.abs().amax(1)) and _bits(cmax, y.abs().amax(0))
    for want, kw in ((UNSUPPORTED_SHAPE, dict(rows=9, c=2052)), (UNSUPPORTED_SHAPE, dict(rows=9, c=30)),
                     (UNSUPPORTED_SHAPE, dict(rows=9, c=64, lead_x=LEAD4)),
                     (INVALID_VALUE, dict(rows=9, c=64, null=True))):
        st, y, rmax, cmax, _ = call(**kw)
        assert st == want, (kw, st)
        assert torch.isnan(y).all() and torch.isnan(rmax).all() and torch.isnan(cmax).all(), kw


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 32, 32), (3, 33, 31), (2, 161, 65)])
def test_nct_to_tnc_in_poison(dev, shape):
    n, c, t = shape
    g = torch.Generator().manual_seed(n * c * t)
    x = torch.randn(n, c, t, generator=g)
    xp, y = Poisoned(x, dev), Poisoned((t, n, c), dev)
    assert _lib.load().ds2_nct_to_tnc(xp.ptr, n, c, t, y.ptr, None) == OK
    torch.cuda.synchronize()
    assert y.intact() and _bits(y.read(), x.permute(2, 0, 1).contiguous())


def test_nct_to_tnc_rejects_a_batch_past_the_grid(dev):
    """n is the grid's z extent (at most 65535): rejected before any launch."""
    assert _lib.load().ds2_nct_to_tnc(None, 65536, 4, 4, None, None) == INVALID_VALUE
    torch.cuda.synchronize()
