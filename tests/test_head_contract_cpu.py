"""CPU: the tables, references and bounds of the head contract tests (head_common, run on the
GPU by test_gpu_head_contract.py) and every status code of the entry points they cover.  The
lookahead table reaches the tile, lane and length edges its rows claim, by the kernels'
constants restated in head_common; the reference's clamp mask is decided with room to spare;
float32 torch on the CPU stays within the a-priori bounds; the greedy and edit-distance
references agree with independent restatements; every refusal returns before any HIP call, so
the pointers handed over here are never dereferenced (0x1000 stands for "not NULL")."""
import numpy as np
import pytest

import torch
from ds2amd import _lib
from ds2amd.decoder import _levenshtein
from oracle import ds2_oracle as orc

import head_common as hc
from head_common import INVALID_VALUE, LA_CASES, OK, UNSUPPORTED_SHAPE, WORKSPACE_TOO_SMALL

P = 0x1000      # a non-NULL pointer no call below reaches far enough to use


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------
# lookahead: the table

def test_the_lookahead_table_reaches_the_edges_its_rows_claim():
    tt, ttw, maxc = hc.LA_TT, hc.LA_TTW, hc.LA_MAXC
    units, ngroups, block = hc.LA_DW_UNITS, hc.LA_DW_NGROUPS, hc.LA_COL_BLOCK
    t, n, h, c = LA_CASES["A"]
    assert c + 1 == maxc and t == tt + 1 == 2 * ttw + 1
    assert h == units + 1 and _cdiv(h, units) == 2 and n == ngroups - 1
    t, n, h, c = LA_CASES["B"]
    assert t == tt and h == units and n == ngroups + 1 and len(range(0, n, ngroups)) == 2
    assert n * h == block + 64 and _cdiv(n * h, block) == 2
    t, n, h, c = LA_CASES["C"]
    assert c == 1 and t == ttw and n * h == 2 * block
    t, n, h, c = LA_CASES["D"]
    assert n == 1 and n * h == block + 1 and _cdiv(h, units) == 5 and t == ttw + 1
    t, n, h, c = LA_CASES["E"]
    assert t < c == maxc - 1
    t, n, h, c = LA_CASES["F"]
    assert c == 20 and t == 2 * tt + 1 and c > 1          # row 32's dx reads dz of rows 12..32
    t, n, h, c = LA_CASES["G"]
    assert n == 2 * ngroups + 1 and h < 64
    # over the table: T on, one past and below a tile of each kernel; the refused context is 32
    ts = {cfg[0] for cfg in LA_CASES.values()}
    assert {tt, tt + 1, ttw, ttw + 1} <= ts and min(ts) < ttw
    assert all(1 <= cfg[3] < maxc for cfg in LA_CASES.values())


def test_the_lookahead_workspace_is_one_partial_per_dw_tile():
    for cfg in LA_CASES.values():
        t, n, h, c = cfg
        assert hc.la_ws_bytes(cfg) == _cdiv(t, hc.LA_TTW) * h * (c + 1) * 4 + 256


@pytest.mark.parametrize("case", list(LA_CASES))
def test_the_clamp_mask_of_the_reference_is_decided_with_room(case):
    """No pre-clamp value of the reference lies within its own bound 2 of 0 or 20, so a device
    result within bound 2 has the reference's inside mask on every element; and 55-80 % of the
    elements are strictly inside, so both sides of the mask are exercised."""
    r = hc.la_ref(case, True)
    lo, hi = hc.LA_CLAMP
    margin = (torch.minimum((r.z - lo).abs(), (r.z - hi).abs()) / r.y_bound).min().item()
    frac = r.inside.double().mean().item()
    print(f"{case}: nearest pre-clamp value {margin:.1f} bounds from a clamp edge, {100 * frac:.0f} % inside")
    assert margin > 1
    assert 0.55 <= frac <= 0.80
    assert torch.equal(r.y, r.z.clamp(lo, hi))
    assert torch.equal(hc.la_ref(case, False).y, r.z)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("case", list(LA_CASES))
def test_float32_cpu_torch_stays_within_the_lookahead_bound(case, clamp):
    """The evidence that bound 2 is not too tight: an independent float32 implementation."""
    r = hc.la_ref(case, clamp)
    print(f"{case} clamp={clamp}: float32 CPU err / bound 2: " +
          "  ".join(f"{k} {v:.3f}" for k, v in r.cpu32.items()))
    assert all(v <= 1 for v in r.cpu32.values()), r.cpu32
    assert (r.y_mag > 0).all() and (r.y_bound > 0).all()


def test_the_integer_case_is_exact_in_float32_and_sits_on_the_clamp_edges():
    for clamp in (False, True):
        r = hc.la_int_ref("A", clamp)
        for v in (r.x, r.w, r.dy, r.z, r.dx, r.dw):
            assert torch.equal(v, v.round())
        # every partial sum of absolute values is an integer below 2^24: exact in any order
        assert max(r.y_mag.max(), r.dx_mag.max(), r.dw_mag.max()).item() < 2 ** 24
        assert all(v == 0 for v in r.cpu32.values()), r.cpu32
    assert int((r.z == 0).sum()) >= 10 and int((r.z == 20).sum()) >= 10
    # Hardtanh's strict test: no gradient through an output exactly at lo or hi
    assert not r.inside[(r.z == 0) | (r.z == 20)].any()


# ------------------------------------------------------------------------------------------
# lookahead: status codes

def _la_fwd(x=P, t=4, n=2, h=3, w=P, context=2, y=P):
    return _lib.load().ds2_lookahead_fwd(x, t, n, h, w, context, 0, 0.0, 0.0, y, None)


def _la_bwd(dy=P, y=None, x=P, t=4, n=2, h=3, w=P, context=2, dx=None, dw=P, ws=None, ws_bytes=0):
    return _lib.load().ds2_lookahead_bwd(dy, y, 0.0, 20.0, x, t, n, h, w, context, dx, dw, ws,
                                         ws_bytes, None)


def test_lookahead_status_codes():
    for call in (_la_fwd, _la_bwd):
        assert call(context=0) == INVALID_VALUE
        assert call(context=-1) == INVALID_VALUE
        assert call(context=hc.LA_MAXC) == UNSUPPORTED_SHAPE
        for k in ("t", "n", "h"):
            assert call(**{k: -1}) == INVALID_VALUE
        # t n h 4 bytes: 2^31 and exactly 2^31 - 64 are past what the 32-bit offsets address
        assert call(t=1 << 15, n=1 << 7, h=1 << 7) == UNSUPPORTED_SHAPE
        assert call(t=16, n=1, h=(1 << 25) - 1) == UNSUPPORTED_SHAPE
    # a negative size comes before the context's range, the range before the empty shape
    assert _la_fwd(t=-1, context=40) == INVALID_VALUE and _la_fwd(t=0, context=40) == UNSUPPORTED_SHAPE
    for k in ("x", "w", "y"):
        assert _la_fwd(**{k: None}) == INVALID_VALUE
    for k in ("t", "n", "h"):
        assert _la_fwd(x=None, w=None, y=None, **{k: 0}) == OK
    # backward: dy and w always, x when dw is asked for; then the workspace, needed for dw only
    assert _la_bwd(dy=None) == INVALID_VALUE
    assert _la_bwd(w=None) == INVALID_VALUE
    assert _la_bwd(x=None) == INVALID_VALUE
    need = hc.la_ws_bytes((4, 2, 3, 2))
    assert _la_bwd(ws=None, ws_bytes=need) == WORKSPACE_TOO_SMALL
    assert _la_bwd(ws=P, ws_bytes=need - 1) == WORKSPACE_TOO_SMALL
    assert _la_bwd(dy=None, x=None, w=None, dw=None, h=0) == OK
    assert _la_bwd(dy=None, x=None, w=None, dw=None, t=0) == OK      # nothing to zero either
    assert _la_bwd(dy=None, x=None, w=None, dw=None, n=0) == OK


# ------------------------------------------------------------------------------------------
# greedy decode

def test_the_greedy_reference_on_the_hand_batch():
    probs, seq = hc.greedy_batch()
    assert probs.shape == (9, 130, 5) and len(hc.GREEDY_SIZES) == 9
    ids, offs, counts, am = hc.greedy_ref(probs, hc.GREEDY_SIZES, 0)
    assert np.array_equal(am[:7], seq)
    # torch.max's index: the first maximum, the first NaN
    assert np.array_equal(am, torch.max(torch.from_numpy(probs), 2)[1].numpy())
    edge = lambda i: [(f, v) for f, v in zip(offs[i], ids[i]) if 60 <= f < 70]
    assert edge(0) == [(62, 2)]                        # held over 62..65: once, at 62
    assert edge(1) == [(63, 3), (65, 3)]               # a blank between: twice
    assert edge(2) == [(63, 3), (64, 1)]
    assert offs[1][-2:] == [128, 129]                  # size 200 is t_max
    assert max(offs[3]) == 63 and max(offs[4]) == 64 and 64 not in offs[3]
    assert counts[5] == 0 and counts[6] == 0           # sizes 0 and -3
    assert counts.tolist() == [len(v) for v in ids] and all(c > 0 for c in counts[[0, 1, 2, 3, 4, 7, 8]])
    # ties: a frame of equal values is class 0; some frame's maximum is shared and not at class 0
    assert (am[7, 63:66] == 0).all()
    top = probs[7] == probs[7].max(1, keepdims=True)
    assert ((top.sum(1) > 1) & (am[7] > 0)).any() and (am[7] == top.argmax(1)).all()
    # NaN: the first of two wins, also against a larger finite value and from class 0
    assert (am[8, 0::21] == 0).all() and am[8, 3] == 1 and am[8, 64] == 2
    # blank = 4 emits class 0 and drops class 4
    ids4, offs4, counts4, _ = hc.greedy_ref(probs, hc.GREEDY_SIZES, 4)
    assert 0 in ids4[0] and 4 not in ids4[0] and 4 in ids[0]
    full = hc.greedy_ref(probs, None, 0)                 # sizes NULL: rows 3..6 decode alike
    assert full[0][3] == full[0][4] == full[0][5] == full[0][6] and full[2][5] > counts[4]


@pytest.mark.parametrize("blank", [0, 4])
def test_the_greedy_reference_equals_the_oracle_decoder(blank):
    """oracle.greedy_decode (the reference decoder restated) on the NaN-free rows."""
    probs, _ = hc.greedy_batch()
    sizes = [min(max(s, 0), 130) for s in hc.GREEDY_SIZES]
    ids, offs, _, _ = hc.greedy_ref(probs, hc.GREEDY_SIZES, blank)
    labels = "ABC D"        # the oracle wants a space among the labels
    strings, offsets = orc.greedy_decode(torch.from_numpy(probs[:8]), sizes[:8], labels, blank)
    for i in range(8):
        assert strings[i][0] == "".join(labels[k] for k in ids[i]), i
        assert offsets[i][0].tolist() == offs[i], i


def test_greedy_status_codes():
    def call(probs=P, n=2, t=10, c=5, sizes=None, blank=0, ids=P, offs=P, counts=P):
        return _lib.load().ds2_greedy_decode(probs, n, t, c, t * c, c, sizes, blank, ids, offs, counts,
                                             None, None)
    assert call(blank=5) == INVALID_VALUE and call(blank=-1) == INVALID_VALUE
    assert call(c=0, blank=0) == INVALID_VALUE
    assert call(n=-1) == INVALID_VALUE and call(t=-1) == INVALID_VALUE
    for k in ("probs", "ids", "offs", "counts"):
        assert call(**{k: None}) == INVALID_VALUE, k
    assert call(probs=None, ids=None, offs=None, counts=None, n=0) == OK


# ------------------------------------------------------------------------------------------
# edit distance

def test_the_closed_forms_against_levenshtein_at_300():
    rng = np.random.default_rng(3)
    a = rng.integers(1, 21, 300).tolist()
    for k in (0, 1, 7):
        d, s = hc.ed_delete(a, k, rng), hc.ed_replace(a, k, rng, 25)
        assert len(d) == 300 - k and len(s) == 300 and s.count(25) == k
        assert _levenshtein(a, d) == _levenshtein(d, a) == k
        assert _levenshtein(a, s) == _levenshtein(s, a) == k
    # deletions placed at chosen positions, on distinct ids
    u = hc.ed_distinct(300)
    cut = hc.ed_delete_at(u, [63, 64, 127, 255, 299])
    assert len(set(u)) == 300 and hc.SPACE not in u and 25 not in u
    assert _levenshtein(cut, u) == _levenshtein(u, cut) == 5
    # the same over words: one-letter words with spaces between
    w = hc.ed_with_spaces(a, 1)
    assert len(hc.ed_words(w)) == 300 and hc.ed_ref(hc.ed_with_spaces(hc.ed_delete(a, 5, rng), 1), w)[:2] == [5, 5]


def test_the_edit_reference_semantics():
    """get_cer_wer's on strings: words are maximal runs of non-space ids, compared whole."""
    from ds2amd.decoder import Decoder
    from ds2amd.trainer import get_cer_wer
    s = hc.SPACE
    assert hc.ed_ref([], []) == [0, 0, 1, 1]
    assert hc.ed_ref([s, s], [s]) == [0, 0, 1, 1]
    assert hc.ed_ref([1, 2, s, 1, 2, s, 1, 2, 3], [1, 2, s, 1, 2, 3, s, 1, 2, s, 1]) == [2, 2, 4, 8]
    assert hc.ed_words([s, 5, s, s, 6, 7, s]) == [(5,), (6, 7)]
    labels = orc.LABELS
    sp = labels.index(" ")
    dec, rng = Decoder(labels), np.random.default_rng(5)
    to_s = lambda r: "".join(labels[k] for k in r)
    for _ in range(20):
        a = rng.choice([sp, 1, 2, 3], int(rng.integers(0, 40))).tolist()
        b = rng.choice([sp, 1, 2, 3], int(rng.integers(0, 40))).tolist()
        wer, cer, wref, cref = get_cer_wer(dec, to_s(a), to_s(b))
        assert hc.ed_ref(a, b, sp) == [wer, cer, int(wref), int(cref)]


def test_edit_distance_status_codes():
    def call(a=P, stride=10, al=P, b=P, bo=P, bl=P, n=2, out=P, err=P):
        return _lib.load().ds2_edit_distance(a, stride, al, b, bo, bl, n, hc.SPACE, out, err, None)
    assert call(n=-1) == INVALID_VALUE and call(stride=-1) == INVALID_VALUE
    for k in ("a", "al", "b", "bo", "bl", "out", "err"):
        assert call(**{k: None}) == INVALID_VALUE, k
    assert call(a=None, al=None, b=None, bo=None, bl=None, out=None, err=None, n=0) == OK


# ------------------------------------------------------------------------------------------
# reductions, guards, softmax

def test_the_colsum_table_reaches_every_chunk_count_step_and_both_kernels():
    assert [hc.colsum_chunks(r) for r in hc.COLSUM_ROWS] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 64, 64]
    # rows per chunk and row group of the vector kernel's loop (two rows in flight, then one)
    per_group = {_cdiv(r, 4) for r in hc.COLSUM_ROWS if 0 < r <= 5}
    assert per_group == {1, 2}
    assert _cdiv(4097, 64) * 63 < 4097        # the last of 64 chunks is not empty: 2 rows
    base = 4 * hc.LEAD16
    assert base % 16 == 0
    for cols, ld, off, kind in hc.COLSUM_FORMS:
        assert off + cols <= ld
        assert hc.colsum_is_vector(cols, ld, base + 4 * off) == (kind == "vector"), (cols, ld, off)
    cols, ld, off, _ = hc.COLSUM_FORMS[-1]
    assert hc.colsum_is_vector(cols, ld, base) and off % 4 != 0      # scalar by the address alone
    assert _lib.size("ds2_colsum_workspace_size", 4097, 260) == hc.COL_CHUNKS * 260 * 8 + 256
    assert _lib.size("ds2_colsum_workspace_size", 0, 260) == hc.COL_CHUNKS * 260 * 8 + 256


def test_the_grid_stride_shapes_reach_a_second_trip():
    first = hc.GRID_CAP * hc.BLOCK
    rows, dirs, h = hc.DIRSUM_SHAPES[-1]
    assert rows * h == 526593 > first and all(r * hh <= first for r, _, hh in hc.DIRSUM_SHAPES[:-1])
    big = hc.NORM_NUMELS[-1]
    assert big // 4 == 2 * first and big % 4 == 3 and big * 4 < 17 * 2 ** 20
    assert {v % 4 for v in hc.NORM_NUMELS} == {0, 1, 2, 3} and 0 in hc.NORM_NUMELS
    assert first < hc.GUARD_NUMEL < 2 * first
    assert _lib.size("ds2_optim_workspace_size", big) == hc.GRID_CAP * 8


def test_colsum_bound_holds_for_a_float32_sum():
    """float32 CPU torch (a pairwise float32 sum, far coarser than the kernels' fp64) misses
    bound 2 and the float64 sum rounded once meets it: the bound tells the two apart."""
    storage, data, out0 = hc.colsum_inputs(4097, 260, 264, 0)
    for acc in (0, 1):
        ref, bound = hc.colsum_ref(data, out0, acc)
        once = (data.sum(0).float() + out0.float()).double() if acc else data.sum(0).float().double()
        assert ((once - ref).abs() <= bound).all()
    coarse = data.float().sum(0).double()
    ref, bound = hc.colsum_ref(data, out0, 0)
    assert ((coarse - ref).abs() > bound).any()


def test_reduction_status_codes():
    lib = _lib.load()
    need = _lib.size("ds2_colsum_workspace_size", 8, 4)

    def colsum(x=P, rows=8, cols=4, ld=4, out=P, ws=P, ws_bytes=need):
        return lib.ds2_colsum(x, rows, cols, ld, out, 0, ws, ws_bytes, None)
    assert colsum(ld=3) == INVALID_VALUE
    assert colsum(rows=-1) == INVALID_VALUE and colsum(cols=-1, ld=4) == INVALID_VALUE
    assert colsum(ws_bytes=need - 1) == WORKSPACE_TOO_SMALL and colsum(ws=None) == WORKSPACE_TOO_SMALL
    assert colsum(x=None) == INVALID_VALUE and colsum(out=None) == INVALID_VALUE
    assert colsum(x=None, rows=0, out=None) == INVALID_VALUE          # out is written: zeros
    assert colsum(x=None, out=None, ws=None, ws_bytes=0, cols=0, ld=0) == OK

    assert lib.ds2_dirsum(None, 3, 2, 4, P, None) == INVALID_VALUE
    assert lib.ds2_dirsum(P, 3, 2, 4, None, None) == INVALID_VALUE
    assert lib.ds2_dirsum(P, 3, 0, 4, P, None) == INVALID_VALUE
    assert lib.ds2_dirsum(P, -1, 2, 4, P, None) == INVALID_VALUE
    assert lib.ds2_dirsum(None, 0, 2, 4, None, None) == OK
    assert lib.ds2_dirsum(None, 3, 2, 0, None, None) == OK

    nbytes = _lib.size("ds2_optim_workspace_size", 8)
    assert lib.ds2_grad_norm(P + 4, 8, P, P, nbytes, None) == INVALID_VALUE       # 16-byte loads
    assert lib.ds2_grad_norm(P, 8, P, P, nbytes - 1, None) == WORKSPACE_TOO_SMALL
    assert lib.ds2_grad_norm(P, 8, P, None, nbytes, None) == WORKSPACE_TOO_SMALL
    assert lib.ds2_grad_norm(P, 8, None, P, nbytes, None) == INVALID_VALUE
    assert lib.ds2_grad_norm(P, -1, P, P, nbytes, None) == INVALID_VALUE

    assert lib.ds2_nan_guard(None, 8, 1, P, None, None) == INVALID_VALUE
    assert lib.ds2_nan_guard(P, 8, 1, None, None, None) == INVALID_VALUE
    assert lib.ds2_nan_guard(P, -1, 1, P, None, None) == INVALID_VALUE
    assert lib.ds2_nan_guard(None, 0, 1, P, None, None) == OK
    assert lib.ds2_zero_masked(P, None, 8, None, None) == INVALID_VALUE
    assert lib.ds2_zero_masked(None, P, 8, None, None) == INVALID_VALUE
    assert lib.ds2_zero_masked(None, None, 0, None, None) == OK
    assert lib.ds2_scale_by_device_scalar(None, 8, P, None) == INVALID_VALUE
    assert lib.ds2_scale_by_device_scalar(P, 8, None, None) == INVALID_VALUE
    assert lib.ds2_scale_by_device_scalar(None, 0, P, None) == OK


def test_softmax_status_codes():
    lib = _lib.load()
    assert lib.ds2_softmax_tnc(None, 3, 2, 5, P, None) == INVALID_VALUE
    assert lib.ds2_softmax_tnc(P, 3, 2, 5, None, None) == INVALID_VALUE
    assert lib.ds2_softmax_tnc(P, 3, 2, 65, P, None) == UNSUPPORTED_SHAPE
    assert lib.ds2_softmax_tnc(None, 0, 2, 5, None, None) == OK
    assert lib.ds2_softmax_tnc(None, 3, 0, 5, None, None) == OK
    for i in range(3):
        args = [P, P, 3, 2, 5, P, 0, None]
        args[(0, 1, 5)[i]] = None
        assert lib.ds2_softmax_tnc_bwd(*args) == INVALID_VALUE, i
    assert lib.ds2_softmax_tnc_bwd(P, P, 3, 2, 0, P, 0, None) == UNSUPPORTED_SHAPE
    assert lib.ds2_softmax_tnc_bwd(None, None, 0, 2, 5, None, 1, None) == OK
