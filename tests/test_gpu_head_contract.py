"""GPU: the kernels every unidirectional model, training step and reported WER / CER goes
through, against plain float64 references across their calling contracts: the lookahead
convolution (csrc/lookahead.hip) at its tile, context and n-group edges, fused with Hardtanh
and not, through the raw entry points; greedy decode and the edit distances (csrc/ctc.hip) at
their 64-frame and 64-column chunk edges and their length limits; ds2_colsum, ds2_dirsum,
ds2_grad_norm, the NaN guard and ds2_softmax_tnc[_bwd] (csrc/misc.hip) at their chunk-count
steps, float4 tails and second grid-stride trips.  Operands sit inside poisoned allocations,
outputs are pre-filled with NaN (int32: a poison word) between canaries, workspaces have
exactly the query's bytes, held 0xFF and sit between canaries (head_common;
test_head_contract_cpu.py proves the tables and holds the status codes).

Two bounds on every floating-point result (head_common.close, printed with pytest -s): the
project's max |err| <= 1e-5 max |ref|, and an elementwise a-priori bound with u = 2^-24 that
holds for any order of summation: (C + 1) u mag for the lookahead's y and dx, T N u mag for its
dw, 2 u (|ref| + |out0|) + rows 2^-53 sum |x| for colsum, 2 u ref for the gradient norm, with
an exact 0 wherever the magnitude is 0.  Integer outputs are compared bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ds2amd import _lib, ops

import head_common as hc
from head_common import (LA_CASES, LA_CLAMP, OK, U, WORKSPACE_TOO_SMALL, WS_LEAD, Poisoned, Workspace,
                         bits, close, close_global, held, held_i32)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# lookahead

def _la_all(cfg, r, dev, clamp, name):
    """Forward, then the full backward, on Poisoned operands; everything asserted against r.
    Returns (y, dx, dw) on the CPU and the Poisoned operands."""
    x, w, dy = hc.la_operands(r, dev)
    y = hc.run_la_fwd(cfg, x, w, dev, clamp)
    assert y.intact(), f"{name}: a write outside y"
    yv = y.read()
    close(yv, r.y, r.y_bound, f"{name} y", cpu32=r.cpu32["y"])
    if clamp:
        got = (yv > LA_CLAMP[0]) & (yv < LA_CLAMP[1])
        assert torch.equal(got, r.inside), f"{name}: {int((got != r.inside).sum())} elements on the other side of the clamp"
    st, dx, dw, ws = hc.run_la_bwd(cfg, dy, y if clamp else None, x, w, dev)
    assert st == OK
    assert dx.intact() and dw.intact() and ws.intact(), f"{name}: a write outside dx, dw or the workspace"
    close(dx.read(), r.dx, r.dx_bound, f"{name} dx", cpu32=r.cpu32["dx"])
    close(dw.read(), r.dw, r.dw_bound, f"{name} dw", cpu32=r.cpu32["dw"])
    return (yv, dx.read(), dw.read()), (x, w, dy, y if clamp else None)


@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
@pytest.mark.parametrize("case", list(LA_CASES))
def test_lookahead_in_poison(dev, case, clamp):
    """ds2_lookahead_fwd / _bwd on x, w, dy surrounded by NaN, y, dx, dw pre-filled with NaN
    between canaries, a 0xFF-filled workspace of exactly the query's bytes: both bounds, the
    reference's inside mask on every element, and the same dw bits from a workspace that held
    zeros.  A NaN in a result is a read past a tensor or an element never written."""
    cfg = LA_CASES[case]
    name = f"lookahead {case} {'clamp' if clamp else 'plain'}"
    (_, dx, dw), (x, w, dy, y) = _la_all(cfg, hc.la_ref(case, clamp), dev, clamp, name)
    st, dx0, dw0, ws0 = hc.run_la_bwd(cfg, dy, y, x, w, dev, ws_fill=0x00)
    assert st == OK and dx0.intact() and dw0.intact() and ws0.intact()
    assert bits(dw, dw0.read()), f"{name}: dw depends on what the workspace held"
    assert bits(dx, dx0.read())


@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
def test_lookahead_integers_are_exact_and_the_clamp_test_is_strict(dev, clamp):
    """Case A on integers (every partial sum below 2^24): y, dx, dw equal float64's values
    exactly.  Hundreds of pre-clamp values are exactly 0 or 20: Hardtanh passes no gradient
    where y == lo or y == hi, so `<=` for `<` in either kernel's mask changes dx and dw."""
    cfg = LA_CASES["A"]
    r = hc.la_int_ref("A", clamp)
    name = f"lookahead A integers {'clamp' if clamp else 'plain'}"
    (y, dx, dw), _ = _la_all(cfg, r, dev, clamp, name)
    for got, ref, nm in ((y, r.y, "y"), (dx, r.dx, "dx"), (dw, r.dw, "dw")):
        assert torch.equal(got.double(), ref), f"{name}: {nm} differs in {int((got.double() != ref).sum())} elements"
    if clamp:
        on_edge = (r.z == LA_CLAMP[0]) | (r.z == LA_CLAMP[1])
        assert int(on_edge.sum()) >= 20 and torch.equal(y.double()[on_edge], r.z[on_edge])


def test_lookahead_partial_calls(dev):
    """dx only (dw NULL, no workspace) and dw only (dx NULL) give the full call's bits; y == NULL
    ignores the clamp arguments; a workspace one byte short (or NULL) is
    DS2_WORKSPACE_TOO_SMALL with dw untouched."""
    cfg = LA_CASES["A"]
    r, plain = hc.la_ref("A", True), hc.la_ref("A", False)
    (_, dx, dw), (x, w, dy, y) = _la_all(cfg, r, dev, True, "lookahead A partial: full call")
    st, dx1, none, ws = hc.run_la_bwd(cfg, dy, y, x, w, dev, want_dw=False, ws_null=True)
    assert st == OK and none is None and ws is None and dx1.intact() and bits(dx, dx1.read())
    st, none, dw1, ws = hc.run_la_bwd(cfg, dy, y, x, w, dev, want_dx=False)
    assert st == OK and none is None and dw1.intact() and ws.intact() and bits(dw, dw1.read())
    # dx alone does not read x
    st, dx2, _, _ = hc.run_la_bwd(cfg, dy, y, None, w, dev, want_dw=False, ws_null=True)
    assert st == OK and dx2.intact() and bits(dx, dx2.read())

    outs = []
    for clamp_args in (LA_CLAMP, (5.0, 6.0)):
        st, dxu, dwu, ws = hc.run_la_bwd(cfg, dy, None, x, w, dev, clamp=clamp_args)
        assert st == OK and dxu.intact() and dwu.intact() and ws.intact()
        outs.append((dxu.read(), dwu.read()))
    assert bits(outs[0][0], outs[1][0]) and bits(outs[0][1], outs[1][1])
    close(outs[0][0], plain.dx, plain.dx_bound, "lookahead A y == NULL dx")
    close(outs[0][1], plain.dw, plain.dw_bound, "lookahead A y == NULL dw")

    need = hc.la_ws_bytes(cfg)
    for kw in (dict(ws_bytes=need - 1), dict(ws_null=True)):
        st, _, dw2, ws = hc.run_la_bwd(cfg, dy, y, x, w, dev, want_dx=False, **kw)
        assert st == WORKSPACE_TOO_SMALL
        assert torch.isnan(dw2.read()).all() and dw2.intact() and (ws is None or ws.intact())


def test_lookahead_empty_shapes(dev):
    """t == 0 or n == 0 with h > 0: dw becomes the empty sum, exact zeros, and dx is not
    touched; h == 0: nothing is touched.  No operand is read: they are NULL."""
    lib = _lib.load()
    for t, n, h, c in ((0, 3, 65, 31), (33, 0, 65, 31), (0, 0, 7, 1), (4, 2, 0, 5)):
        rows = max(h, 3)
        dx, dw = Poisoned((5, 2, rows), dev), Poisoned((rows, c + 1), dev)
        ws = Workspace(hc.la_ws_bytes((t, n, h, c)), dev)
        st = lib.ds2_lookahead_bwd(None, None, 0.0, 20.0, None, t, n, h, None, c, dx.ptr, dw.ptr,
                                   ws.ptr, ws.nbytes, None)
        assert st == OK
        y = Poisoned((5, 2, rows), dev)
        assert lib.ds2_lookahead_fwd(None, t, n, h, None, c, 1, 0.0, 20.0, y.ptr, None) == OK
        torch.cuda.synchronize()
        assert dx.intact() and dw.intact() and ws.intact() and y.intact()
        assert torch.isnan(dx.read()).all() and torch.isnan(y.read()).all()
        if h:
            assert (dw.read() == 0).all(), "dw of an empty batch is not exact zeros"
        else:
            assert torch.isnan(dw.read()).all()


def test_lookahead_function_on_the_model_context(dev):
    """ops.LookaheadFn through autograd on case F, fused, against the same reference."""
    r = hc.la_ref("F", True)
    xd = r.x.float().to(dev).requires_grad_(True)
    wd = r.w.float().to(dev).requires_grad_(True)
    yd = ops.LookaheadFn.apply(xd, wd, LA_CLAMP)
    yd.backward(r.dy.float().to(dev))
    close(yd, r.y, r.y_bound, "LookaheadFn F y")
    yv = yd.detach().cpu()
    assert torch.equal((yv > LA_CLAMP[0]) & (yv < LA_CLAMP[1]), r.inside)
    close(xd.grad, r.dx, r.dx_bound, "LookaheadFn F dx")
    close(wd.grad, r.dw, r.dw_bound, "LookaheadFn F dw")


# ------------------------------------------------------------------------------------------
# greedy decode

def _greedy(dev, probs, sizes, blank, transposed=False, want_argmax=True):
    ids, offs, counts, am, intact = hc.run_greedy(probs, sizes, blank, dev, transposed, want_argmax)
    rid, roff, rcount, ram = hc.greedy_ref(probs, sizes, blank)
    assert intact, "a write outside ids, offsets, counts or argmax"
    if want_argmax:
        assert np.array_equal(am.numpy(), ram)
    assert counts.tolist() == rcount.tolist()
    for i, k in enumerate(rcount.tolist()):
        assert ids[i, :k].tolist() == rid[i], i
        assert offs[i, :k].tolist() == roff[i], i
        # nothing is written behind the emitted entries
        assert (ids[i, k:] == hc.I32_POISON).all() and (offs[i, k:] == hc.I32_POISON).all(), i
    return rid, roff


@pytest.mark.parametrize("transposed", [False, True], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("with_sizes", [True, False], ids=["sizes", "sizes-null"])
@pytest.mark.parametrize("blank", [0, 4])
def test_greedy_hand_batch(dev, blank, with_sizes, transposed):
    """head_common.greedy_batch: a label held over frames 62..65 is emitted once, at 62 (the
    previous frame's index is carried over the 64-frame chunk edge); a blank between two equal
    labels at 63 and 65 separates them; sizes 64, 65, 0, 200 and -3; ties and NaN."""
    probs, _ = hc.greedy_batch()
    rid, roff = _greedy(dev, probs, hc.GREEDY_SIZES if with_sizes else None, blank, transposed)
    if blank == 0:
        assert [(f, v) for f, v in zip(roff[0], rid[0]) if 60 <= f < 70] == [(62, 2)]
        assert [(f, v) for f, v in zip(roff[1], rid[1]) if 60 <= f < 70] == [(63, 3), (65, 3)]


def test_greedy_one_class_and_a_hundred(dev):
    """c = 1: every frame is the blank, counts 0.  c = 100: more classes than a wave has lanes
    (the argmax is a loop per lane), five rows: a second block."""
    rng = np.random.default_rng(2)
    one = rng.random((3, 70, 1)).astype(np.float32)
    _greedy(dev, one, [70, 10, 0], 0)
    assert hc.greedy_ref(one, None, 0)[2].tolist() == [0, 0, 0]
    wide = rng.random((5, 70, 100)).astype(np.float32)
    wide[:, :, 0] += 0.2
    wide[:, 30:40, 99] = 2.0                      # the last class, held over ten frames
    for blank in (0, 99):
        _greedy(dev, wide, [70, 64, 65, 300, -1], blank)
        _greedy(dev, wide, None, blank, transposed=True, want_argmax=False)


# ------------------------------------------------------------------------------------------
# edit distance

def _ids(rng, n, hi=21):
    return rng.integers(1, hi, n).tolist()


def test_edit_distance_lds_rows_and_empty_sides(dev):
    """Reference lengths 257, 319 and 320 (the LDS DP's row of n + 1 columns in 64-column
    chunks: the last chunk holds 2, 64 and 1 of them) against 300 random ids, words every 6 ids,
    and against themselves with the ids deleted whose insertion falls on a chunk's first lane; an empty side on the register DP (n = 70, n = 0) and the LDS DP (n = 300); both empty;
    a repeated word on both sides and words that differ only in length; a row stride 37 past
    the longest row with -1 in the slack.  Against _levenshtein."""
    rng = np.random.default_rng(23)
    s = hc.SPACE
    a_rows, b_rows = [], []
    for lb in (257, 319, 320):
        a_rows.append(hc.ed_with_spaces(_ids(rng, 300, 5), 6))
        b_rows.append(hc.ed_with_spaces(_ids(rng, lb, 5), 6))
        a_rows.append(_ids(rng, 300, 5))             # one long word each
        b_rows.append(_ids(rng, lb, 5))
    for la, lb in ((0, 70), (0, 300), (300, 0), (0, 0)):
        a_rows.append(_ids(rng, la))
        b_rows.append(_ids(rng, lb))
    # insertions in the first lane of a chunk, and in the chunk that holds column n alone: the
    # minimum of the row so far reaches them only through the carry between chunks
    for lb in (257, 319, 320):
        b_rows.append(hc.ed_distinct(lb))
        a_rows.append(hc.ed_delete_at(b_rows[-1], [63, 64, 255, lb - 1]))
    a_rows.append([s, s])
    b_rows.append(hc.ed_with_spaces(_ids(rng, 300), 3))
    a_rows.append([1, 2, s, 1, 2, s, 1, 2, 3, s, 1, 2])
    b_rows.append([s, 1, 2, s, s, 1, 2, 3, s, 1, 2, s, 1, s, 1, 2])
    out, err, _, intact = hc.run_edit(a_rows, b_rows, dev)
    assert intact and err == 0
    for i, (a, b) in enumerate(zip(a_rows, b_rows)):
        assert out[i].tolist() == hc.ed_ref(a, b), (i, len(a), len(b))
    assert out[9].tolist() == [0, 0, 1, 1]
    assert out[6].tolist() == [1, 70, 1, 70] and out[8].tolist() == [1, 300, 1, 1]
    assert out[10:13].tolist() == [[1, 4, 1, lb] for lb in (257, 319, 320)]


def test_edit_distance_at_the_length_limits(dev):
    """Exactly 2048 non-space ids and exactly 1024 words are accepted, on either side: the LDS
    DP over 33 column chunks, against the closed forms (k ids deleted -- here those whose
    insertion falls on a chunk's first lane --, or k replaced by an id the other side lacks:
    distance k).  500 spaces among the 2048 ids make the raw length 2548:
    the limit counts non-space ids."""
    rng = np.random.default_rng(29)
    full = hc.ed_distinct(hc.ED_MAXC)
    k = 7
    # the deleted ids: the first lane of chunks 2, 3, 17, 18 and 32, a run over a chunk edge, and
    # column 2048, alone in chunk 33
    dele = hc.ed_delete_at(full, [63, 64, 127, 1023, 1087, 1983, 2047])
    repl = hc.ed_replace(full, k, rng, 25)
    assert len(full) == len(repl) == 2048 and len(dele) == 2041
    a_rows = [full, dele, full, repl]
    b_rows = [dele, full, repl, full]
    want = [[1, k, 1, 2041], [1, k, 1, 2048], [1, k, 1, 2048], [1, k, 1, 2048]]
    # 500 spaces, at the same places on both sides
    sp_full, sp_repl = hc.ed_with_spaces(full, 4, limit=500), hc.ed_with_spaces(repl, 4, limit=500)
    assert len(sp_full) == 2548 and sp_full.count(hc.SPACE) == 500
    assert [v for v in sp_full if v != hc.SPACE] == full and [v for v in sp_repl if v != hc.SPACE] == repl
    wa, wb = hc.ed_words(sp_repl), hc.ed_words(sp_full)
    assert len(wa) == len(wb) == 501
    wid = {}
    word_dist = hc._levenshtein([wid.setdefault(v, len(wid)) for v in wa],
                                [wid.setdefault(v, len(wid)) for v in wb])
    assert 1 <= word_dist <= k
    a_rows.append(sp_repl)
    b_rows.append(sp_full)
    want.append([word_dist, k, 501, 2048])
    # 1024 one-letter words, 5 of them deleted on one side
    words = hc.ed_distinct(hc.ED_MAXW)
    fewer = hc.ed_delete_at(words, [63, 64, 511, 959, 1023])
    for a, b, nref in ((words, fewer, 1019), (fewer, words, 1024)):
        a_rows.append(hc.ed_with_spaces(a, 1))
        b_rows.append(hc.ed_with_spaces(b, 1))
        want.append([5, 5, nref, nref])
    out, err, _, intact = hc.run_edit(a_rows, b_rows, dev)
    assert intact and err == 0
    assert out.tolist() == want


def test_edit_distance_past_the_length_limits(dev):
    """2049 non-space ids or 1025 words on either side: *err != 0, both distances -1 and the two
    reference counts still right; a valid pair of the same launch is scored; a second, valid
    launch on the zeroed word leaves it 0."""
    rng = np.random.default_rng(31)
    long_ids = _ids(rng, hc.ED_MAXC + 1)
    many = hc.ed_with_spaces(_ids(rng, hc.ED_MAXW + 1), 1)
    short = hc.ed_with_spaces(_ids(rng, 40), 5)
    other = hc.ed_with_spaces(_ids(rng, 50), 5)
    a_rows = [long_ids, short, many, short, other]
    b_rows = [short, long_ids, short, many, short]
    out, err, word, intact = hc.run_edit(a_rows, b_rows, dev)
    assert intact and err != 0
    nw, nc = len(hc.ed_words(short)), 40
    assert out[:4].tolist() == [[-1, -1, nw, nc], [-1, -1, 1, 2049], [-1, -1, nw, nc], [-1, -1, 1025, 1025]]
    assert out[4].tolist() == hc.ed_ref(other, short)
    word.view.zero_()
    out, err, _, intact = hc.run_edit([other, short], [short, other], dev, err=word)
    assert intact and err == 0
    assert out.tolist() == [hc.ed_ref(other, short), hc.ed_ref(short, other)]


# ------------------------------------------------------------------------------------------
# reductions

@pytest.mark.parametrize("cols,ld,off,kind", hc.COLSUM_FORMS,
                         ids=[f"{c}-{l}-{o}-{k}" for c, l, o, k in hc.COLSUM_FORMS])
def test_colsum_in_poison(dev, cols, ld, off, kind):
    """Every row count of head_common.COLSUM_ROWS (1..5 rows in the vector kernel's
    two-rows-in-flight loop, the chunk-count steps, 0), accumulate 0 and 1: the data inside
    NaN -- the ld - cols slack columns too --, out holding out0 between canaries, the query's
    workspace; both bounds; integers exactly."""
    for rows in hc.COLSUM_ROWS:
        storage, data, out0 = hc.colsum_inputs(rows, cols, ld, off)
        for acc in (0, 1):
            got, addr, intact = hc.run_colsum(storage, rows, cols, ld, off, out0, acc, dev)
            assert hc.colsum_is_vector(cols, ld, addr) == (kind == "vector")
            assert intact, "a write outside out or outside the workspace"
            ref, bound = hc.colsum_ref(data, out0, acc)
            close(got, ref, bound, f"colsum {kind} {rows}x{cols} ld {ld} off {off} acc {acc}")
            if rows == 0:
                assert torch.equal(got.double(), out0 if acc else torch.zeros(cols, dtype=torch.float64))
    for rows in (5, 129, 4097):
        storage, data, out0 = hc.colsum_inputs(rows, cols, ld, off, integer=True)
        for acc in (0, 1):
            got, _, intact = hc.run_colsum(storage, rows, cols, ld, off, out0, acc, dev, ws_fill=0x00)
            assert intact and torch.equal(got.double(), hc.colsum_ref(data, out0, acc)[0])


@pytest.mark.parametrize("rows,dirs,h", hc.DIRSUM_SHAPES)
def test_dirsum_in_poison(dev, rows, dirs, h):
    """(2049, 2, 257): 526 593 outputs, past the 2048 x 256 of the grid-stride loop's first
    trip.  Integers exactly; floats to one rounding per addition, (dirs - 1) u sum |x|."""
    g = torch.Generator().manual_seed(rows * h + dirs)
    for integer in (True, False):
        x = (torch.randint(-100, 101, (rows, dirs, h), generator=g).double() if integer else
             torch.randn(rows, dirs, h, generator=g, dtype=torch.float64).float().double())
        xp, y = Poisoned(x, dev), Poisoned((rows, h), dev)
        assert _lib.load().ds2_dirsum(xp.ptr, rows, dirs, h, y.ptr, None) == OK
        torch.cuda.synchronize()
        assert y.intact(), "a write outside y"
        ref = x.sum(1)
        if integer or dirs == 1:
            assert torch.equal(y.read().double(), ref)
        else:
            close(y.read(), ref, (dirs - 1) * U * x.abs().sum(1), f"dirsum {rows}x{dirs}x{h}")


def test_grad_norm_tails_and_second_trip(dev):
    """numel 0 (exactly 0), float4 tails of 0..3 elements, and 2 x 2048 x 256 float4 + 3: the
    second trip of the float4 loop and a scalar tail, 16 MB.  NaN follows the last element.
    fp64 sums, one rounding of the root and one of the result: 2 u ref."""
    for numel in hc.NORM_NUMELS:
        x = hc.norm_input(numel)
        got, intact = hc.run_grad_norm(x, dev)
        assert intact
        ref = (x.double() ** 2).sum().sqrt().item()
        if numel == 0:
            assert got == 0.0
            continue
        frac = abs(got - ref) / (2 * U * ref)
        print(f"HEAD_CONTRACT grad_norm {numel}: global err / bound = {abs(got - ref) / (1e-5 * ref):.3f}  "
              f"elementwise err / bound = {frac:.3f}")
        assert np.isfinite(got) and frac <= 1, (numel, got, ref)


def _guard_input():
    n = hc.GUARD_NUMEL
    x = torch.randn(n, generator=torch.Generator().manual_seed(41))
    where = [0, 12345, hc.GRID_CAP * hc.BLOCK + 1, n - 1]     # the last two: the second trip
    return x, where


@pytest.mark.parametrize("zero_nans", [0, 1])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "mask-null"])
def test_nan_guard_second_trip(dev, zero_nans, with_mask):
    """numel = 2048 x 256 + 5: NaN at index 0, in the first trip, in the second and at the last
    index.  The flag, every mask byte (the mask held 7s), and x zeroed or left as it was."""
    x, where = _guard_input()
    n = x.numel()
    lib = _lib.load()
    for poisoned in (True, False):
        src = x.clone()
        if poisoned:
            src[where] = float("nan")
        xp, flag = held(src, dev), held_i32(torch.zeros(1), dev)
        mask = Workspace(n, dev, fill=7) if with_mask else None
        st = lib.ds2_nan_guard(xp.ptr, n, zero_nans, flag.ptr, None if mask is None else mask.ptr, None)
        assert st == OK
        torch.cuda.synchronize()
        assert xp.intact() and flag.intact() and (mask is None or mask.intact())
        assert flag.read().item() == int(poisoned)
        want = src.clone()
        if zero_nans and poisoned:
            want[where] = 0.0
        assert bits(xp.read(), want)
        if mask is not None:
            m = mask.buf[WS_LEAD:WS_LEAD + n].cpu()
            assert m.sum().item() == (len(where) if poisoned else 0) and m.max().item() <= 1
            assert (m[where] == int(poisoned)).all()


def test_zero_masked_and_scale_second_trip(dev):
    """ds2_zero_masked: a no-op under a clear flag, acts under a set flag and under flag ==
    NULL.  ds2_scale_by_device_scalar by 0.25 is exact.  Both at 2048 x 256 + 5 elements."""
    x, where = _guard_input()
    n = x.numel()
    lib = _lib.load()
    mask_host = torch.zeros(n, dtype=torch.uint8)
    mask_host[where] = 1
    zeroed = x.clone()
    zeroed[where] = 0.0
    for flag_value, want in ((0, x), (1, zeroed), (None, zeroed)):
        xp = held(x, dev)
        mask = Workspace(n, dev, fill=0)
        mask.buf[WS_LEAD:WS_LEAD + n].copy_(mask_host)
        flag = None if flag_value is None else held_i32(torch.tensor([flag_value]), dev)
        st = lib.ds2_zero_masked(xp.ptr, mask.ptr, n, None if flag is None else flag.ptr, None)
        assert st == OK
        torch.cuda.synchronize()
        assert xp.intact() and bits(xp.read(), want), flag_value
        assert torch.equal(mask.buf[WS_LEAD:WS_LEAD + n].cpu(), mask_host)
    xp, s = held(x, dev), Poisoned(torch.tensor([0.25]), dev)
    assert lib.ds2_scale_by_device_scalar(xp.ptr, n, s.ptr, None) == OK
    torch.cuda.synchronize()
    assert xp.intact() and bits(xp.read(), x * 0.25)


# ------------------------------------------------------------------------------------------
# softmax

@pytest.mark.parametrize("t,n,c", [(7, 3, 29), (5, 2, 63)])
def test_softmax_tnc_in_poison(dev, t, n, c):
    """test_gpu_ops._softmax_tnc_case's shapes through the raw entry points: logits [T][N][C]
    inside NaN, the transposed probs [N][T][C] and dlogits pre-filled with NaN between canaries
    (a wrong row index writes into another utterance's rows or just past the tensor), the
    backward overwriting and accumulating; the existing bounds, 1e-6 and 1e-5."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(t, n, c, generator=g, dtype=torch.float64) * 4).float().double()
    dp = torch.randn(n, t, c, generator=g, dtype=torch.float64).float().double()
    dst0 = torch.randn(t, n, c, generator=g, dtype=torch.float64).float().double()
    xr = x.clone().requires_grad_(True)
    ref = F.softmax(xr.transpose(0, 1), -1)
    ref.backward(dp)
    xp, probs = Poisoned(x, dev), Poisoned((n, t, c), dev)
    assert lib.ds2_softmax_tnc(xp.ptr, t, n, c, probs.ptr, None) == OK
    torch.cuda.synchronize()
    assert probs.intact(), "a write outside probs"
    close_global(probs.read(), ref.detach(), 1e-6, f"softmax {t}x{n}x{c}")
    pin, dpp = Poisoned(probs.read(), dev), Poisoned(dp, dev)
    for acc, want in ((0, xr.grad), (1, dst0 + xr.grad)):
        dl = held(dst0, dev) if acc else Poisoned((t, n, c), dev)
        assert lib.ds2_softmax_tnc_bwd(pin.ptr, dpp.ptr, t, n, c, dl.ptr, acc, None) == OK
        torch.cuda.synchronize()
        assert dl.intact(), "a write outside dlogits"
        close_global(dl.read(), want, 1e-5, f"softmax bwd {t}x{n}x{c} accumulate {acc}")
