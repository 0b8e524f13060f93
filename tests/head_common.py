"""Helpers of the head contract tests (test_gpu_head_contract.py, test_head_contract_cpu.py):
the lookahead convolution (csrc/lookahead.hip), greedy decode and the edit distances
(csrc/ctc.hip), and the reductions, guards and softmax of csrc/misc.hip.  The case tables with
the kernels' tile constants restated, input generators, plain float64 references with the
magnitude of every sum, the two bounds, and runners that call the C entry points directly on
operands inside poisoned allocations (conv_common.Poisoned, PoisonedI32 here) with workspaces
of exactly the query's bytes between canaries (conv_common.Workspace)."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from ds2amd import _lib
from ds2amd.decoder import _levenshtein
from oracle import ds2_oracle as orc

from conv_common import CANARY, LEAD16, TAIL, WS_LEAD, Poisoned, Workspace  # noqa: F401  (re-exported)

OK, INVALID_VALUE, UNSUPPORTED_SHAPE, WORKSPACE_TOO_SMALL = 0, 1, 2, 5
U = 2.0 ** -24          # float32 unit roundoff
GLOBAL_REL = 1e-5       # test_gpu_ops._close: max |err| <= 1e-5 max |ref|


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def held(data, dev, lead=LEAD16):
    """A Poisoned output allocation (canaries around it) that holds `data`: an operand the
    call updates in place, or an output under accumulate."""
    p = Poisoned(tuple(data.shape), dev, lead)
    p.view.copy_(data.float())
    return p


I32_POISON = -0x21524111    # what an int32 output holds before the call
I32_JUNK = 0x7F7F7F7F       # what surrounds an int32 input


class PoisonedI32:
    """conv_common.Poisoned for int32: an input (a CPU tensor is given) sits in I32_JUNK, an
    output (a shape is given) holds I32_POISON and sits in the canary word.  All of it is live
    memory."""

    def __init__(self, data_or_shape, dev, lead=LEAD16):
        is_input = isinstance(data_or_shape, torch.Tensor)
        self.shape = tuple(data_or_shape.shape) if is_input else tuple(data_or_shape)
        self.numel = int(np.prod(self.shape, dtype=np.int64))
        self.lead = lead
        host = torch.full((lead + self.numel + TAIL,), I32_JUNK if is_input else CANARY, dtype=torch.int32)
        host[lead:lead + self.numel] = data_or_shape.reshape(-1).to(torch.int32) if is_input else I32_POISON
        self.is_input = is_input
        self.buf = host.to(dev)
        assert self.buf.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lead

    @property
    def view(self):
        return self.buf[self.lead:self.lead + self.numel].view(self.shape)

    def read(self):
        return self.view.cpu()

    def intact(self):
        assert not self.is_input
        return bool((self.buf[:self.lead] == CANARY).all().item() and
                    (self.buf[self.lead + self.numel:] == CANARY).all().item())


def held_i32(data, dev):
    p = PoisonedI32(tuple(data.shape), dev)
    p.view.copy_(data.to(torch.int32))
    return p


def close(got, ref, bound, name, rel=GLOBAL_REL, cpu32=None):
    """Bound 1: max |err| <= rel max |ref|.  Bound 2: |err| <= bound elementwise (a tensor, the
    a-priori bound of the operation), and got == 0 exactly where bound == 0.  Prints both errors
    as fractions of their bounds before it asserts; cpu32: float32 CPU torch's fraction of
    bound 2 on the same inputs."""
    got, ref, bound = (v.detach().double().cpu() for v in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output (a read past a tensor, or an element never written)"
    err = (got - ref).abs()
    emax = err.max().item() if err.numel() else 0.0
    scale = max(ref.abs().max().item() if ref.numel() else 0.0, 1e-30)
    g = emax / (rel * scale)
    zero = bound == 0
    frac = (err / bound.clamp_min(1e-300))[~zero]
    c = frac.max().item() if frac.numel() else 0.0
    tail = "" if cpu32 is None else f"  cpu float32 elementwise {cpu32:.3f}"
    print(f"HEAD_CONTRACT {name}: global err / bound = {g:.3f}  elementwise err / bound = {c:.3f}{tail}")
    assert g <= 1, f"{name}: max err {emax:.3e} > {rel:.0e} * {scale:.3e}"
    assert c <= 1, f"{name}: an element is {c:.3f} x its a-priori bound off"
    assert (got[zero] == 0).all(), f"{name}: a sum of exact zeros is not exactly 0"


def close_global(got, ref, rel, name):
    """Bound 1 alone (softmax: 1e-6 forward, 1e-5 backward, as test_gpu_ops has them)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    print(f"HEAD_CONTRACT {name}: global err / bound = {err / (rel * scale):.3f}")
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.0e} * {scale:.3e}"


# ------------------------------------------------------------------------------------------
# lookahead

# csrc/lookahead.hip: time steps per thread of the forward and dx kernels, of the dw partial
# kernel, the register arrays' length (context + 1 <= LA_MAXC), and the launch geometry
LA_TT, LA_TTW, LA_MAXC = 32, 16, 32
LA_DW_UNITS, LA_DW_NGROUPS, LA_COL_BLOCK = 64, 4, 256
LA_CLAMP = (0.0, 20.0)

# id -> (T, N, H, context); what each is there for: test_head_contract_cpu.py asserts it
LA_CASES = {
    # context + 1 = LA_MAXC; T = one 32-tile + 1 = two 16-tiles + 1; H = 64 + 1: a second dw block
    # holding one unit; N = 3: n-group 3 is empty
    "A": (33, 3, 65, 31),
    # T exactly one tile; H exactly one dw block; N = 5: group 0 takes two samples; 320 columns =
    # one full 256-thread block and a partial one
    "B": (32, 5, 64, 20),
    # the smallest context; T = one dw tile; 512 columns = exactly two blocks
    "C": (16, 4, 128, 1),
    # one column in the last of two column blocks; five dw blocks; N = 1
    "D": (17, 1, 257, 2),
    # T < context: every output reads the zero padding
    "E": (5, 2, 7, 31),
    # the model's context; two 32-tiles + 1: the dx window reaches back across a tile edge
    "F": (65, 2, 40, 20),
    # N = 9 over 4 n-groups; H far below a wave
    "G": (49, 9, 3, 7),
}

LaRef = collections.namedtuple(
    "LaRef", "x w dy z y inside dx dw y_mag dx_mag dw_mag y_bound dx_bound dw_bound cpu32")


def _la_results(x, w, dy, clamp):
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    z = orc.lookahead(xr, wr)
    y = F.hardtanh(z, *LA_CLAMP) if clamp else z
    y.backward(dy)
    return z.detach(), y.detach(), xr.grad, wr.grad


def la_inputs(cfg):
    """test_lookahead's generator at seed 1000 + 31 T + H, every value rounded to float32 (what
    the device holds), as float64."""
    t, n, h, c = cfg
    g = torch.Generator().manual_seed(1000 + 31 * t + h)
    x = (torch.randn(t, n, h, generator=g, dtype=torch.float64) * 8 + 4).float().double()
    w = (torch.rand(h, c + 1, generator=g, dtype=torch.float64) - 0.3).float().double()
    dy = torch.randn(t, n, h, generator=g, dtype=torch.float64).float().double()
    return x, w, dy


def la_int_inputs(cfg, seed=5):
    """Integers: x, dy in [-3, 3], w in [-2, 2].  Every partial sum is an integer far below
    2^24, so float32 is exact in any order."""
    t, n, h, c = cfg
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (t, n, h), generator=g).double()
    w = torch.randint(-2, 3, (h, c + 1), generator=g).double()
    dy = torch.randint(-3, 4, (t, n, h), generator=g).double()
    return x, w, dy


def _la_ref(cfg, clamp, x, w, dy):
    t, n, h, c = cfg
    z, y, dx, dw = _la_results(x, w, dy, clamp)
    inside = (z > LA_CLAMP[0]) & (z < LA_CLAMP[1]) if clamp else torch.ones_like(z, dtype=torch.bool)
    # the same sums over absolute values; the backward's under the reference's inside mask
    xa, wa = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    za = orc.lookahead(xa, wa)
    za.backward(dy.abs() * inside)
    mags = (za.detach(), xa.grad, wa.grad)
    bounds = ((c + 1) * U * mags[0], (c + 1) * U * mags[1], t * n * U * mags[2])
    _, y32, dx32, dw32 = _la_results(x.float(), w.float(), dy.float(), clamp)
    cpu32 = {k: ((a.double() - r).abs() / b.clamp_min(1e-300))[b > 0].max().item()
             for k, a, r, b in zip(("y", "dx", "dw"), (y32, dx32, dw32), (y, dx, dw), bounds)}
    return LaRef(x, w, dy, z, y, inside, dx, dw, *mags, *bounds, cpu32)


@functools.lru_cache(maxsize=None)
def la_ref(case, clamp):
    """Float64 reference of a table case (oracle.lookahead, hardtanh, autograd), the magnitudes,
    bound 2 of each result -- (C + 1) u mag for y and dx (a sum of C + 1 products), T N u mag for
    dw (a sum of T N products), in any order of summation, fused or not -- and float32 CPU
    torch's worst fraction of it.  Shared: never modify the tensors."""
    return _la_ref(LA_CASES[case], clamp, *la_inputs(LA_CASES[case]))


@functools.lru_cache(maxsize=None)
def la_int_ref(case, clamp):
    return _la_ref(LA_CASES[case], clamp, *la_int_inputs(LA_CASES[case]))


def la_ws_bytes(cfg):
    return _lib.size("ds2_lookahead_bwd_workspace_size", *cfg)


def la_operands(r, dev):
    return Poisoned(r.x, dev), Poisoned(r.w, dev), Poisoned(r.dy, dev)


def run_la_fwd(cfg, x, w, dev, clamp):
    """ds2_lookahead_fwd on Poisoned x, w.  Returns the Poisoned y (NaN where never written)."""
    t, n, h, c = cfg
    y = Poisoned((t, n, h), dev)
    lo, hi = LA_CLAMP if clamp else (0.0, 0.0)
    st = _lib.load().ds2_lookahead_fwd(x.ptr, t, n, h, w.ptr, c, int(bool(clamp)), lo, hi, y.ptr, None)
    _lib.check(st, "ds2_lookahead_fwd")
    torch.cuda.synchronize()
    return y


def run_la_bwd(cfg, dy, y, x, w, dev, clamp=LA_CLAMP, want_dx=True, want_dw=True, ws_fill=0xFF,
               ws_bytes=None, ws_null=False):
    """ds2_lookahead_bwd on Poisoned operands; y: the Poisoned clamped output or None (unfused:
    the clamp arguments are then ignored).  The workspace is ws_bytes (default: the query's)
    bytes of ws_fill between canaries, or NULL and 0 bytes.  Returns (status, dx, dw, ws): the
    Poisoned outputs asked for (else None) and the Workspace."""
    t, n, h, c = cfg
    dx = Poisoned((t, n, h), dev) if want_dx else None
    dw = Poisoned((h, c + 1), dev) if want_dw else None
    ws = None if ws_null else Workspace(la_ws_bytes(cfg) if ws_bytes is None else ws_bytes, dev, ws_fill)
    st = _lib.load().ds2_lookahead_bwd(
        dy.ptr, None if y is None else y.ptr, clamp[0], clamp[1], None if x is None else x.ptr,
        t, n, h, w.ptr, c, None if dx is None else dx.ptr, None if dw is None else dw.ptr,
        None if ws is None else ws.ptr, 0 if ws is None else ws.nbytes, None)
    torch.cuda.synchronize()
    return st, dx, dw, ws


# ------------------------------------------------------------------------------------------
# greedy decode

GREEDY_CHUNK = 64       # frames per pass of greedy_kernel's wave


def greedy_ref(probs, sizes, blank):
    """probs [n][t][c] (numpy).  The first maximum, a NaN counting as the maximum and the first
    NaN winning; blanks and frames equal to the previous frame's index dropped; only frames
    below clamp(size, 0, t) emitted.  Returns (ids, offsets) as lists per row, counts, argmax."""
    n, t, c = probs.shape
    nan = np.isnan(probs)
    argmax = np.where(nan.any(2), nan.argmax(2), np.where(nan, -np.inf, probs).argmax(2)).astype(np.int32)
    ids, offs = [], []
    for i in range(n):
        size = t if sizes is None else min(max(int(sizes[i]), 0), t)
        keep = [f for f in range(size)
                if argmax[i, f] != blank and not (f > 0 and argmax[i, f] == argmax[i, f - 1])]
        ids.append([int(argmax[i, f]) for f in keep])
        offs.append(keep)
    return ids, offs, np.array([len(k) for k in ids], dtype=np.int32), argmax


GREEDY_SIZES = [130, 200, 130, 64, 65, 0, -3, 130, 130]


def greedy_batch():
    """n = 9, t_max = 130, c = 5, written by hand.  Returns (probs, the argmax sequences of
    rows 0..6 as written).
    row 0: label 2 held over frames 62..65 (one emission, at 62, carried over the chunk edge)
    row 1: label 3 at 63, class 0 at 64, label 3 at 65 (two emissions under blank 0); size 200
    row 2: label 3 at 63, label 1 at 64
    rows 3..6: labels alternating over frames 60..69, sizes 64, 65, 0 and -3
    row 7: ties (values on a grid of three; whole frames equal)
    row 8: NaN in two classes of a frame (every third), in classes 0 and 4 (every seventh)"""
    n, t, c = 9, 130, 5
    rng = np.random.default_rng(11)
    probs = (rng.random((n, t, c)) * 0.5).astype(np.float32)
    seq = np.zeros((7, t), dtype=np.int64)
    seq[:, 5:7] = 1
    seq[:, 100] = 3
    seq[:, 128] = 4
    seq[:, 129] = 2
    seq[0, 62:66] = 2
    seq[1, 63], seq[1, 64], seq[1, 65] = 3, 0, 3
    seq[2, 63], seq[2, 64] = 3, 1
    seq[3:7, 60:70] = np.array([1, 2, 1, 2, 3, 3, 1, 4, 4, 1])
    for i in range(7):
        probs[i, np.arange(t), seq[i]] = 0.9
    probs[7] = rng.integers(0, 3, (t, c)).astype(np.float32) * 0.25
    probs[7, 63:66] = 0.25
    probs[8, np.arange(t), rng.integers(0, c, t)] = 0.9
    probs[8, 0::3, 1] = np.nan
    probs[8, 0::3, 3] = np.nan
    probs[8, 0::7, 0] = np.nan
    probs[8, 0::7, 4] = np.nan
    probs[8, 64, 2] = np.nan
    return probs, seq


def run_greedy(probs, sizes, blank, dev, transposed=False, want_argmax=True):
    """ds2_greedy_decode on probs [n][t][c] (numpy) inside NaN, outputs in int32 poison and
    canary.  transposed: the device holds [t][n][c] (stride_t = n c, stride_n = c).  Returns
    (ids [n][t], offsets [n][t], counts [n], argmax [n][t] or None) on the CPU and whether
    every canary is intact."""
    n, t, c = probs.shape
    pt = torch.from_numpy(probs)
    p = Poisoned(pt.permute(1, 0, 2).contiguous() if transposed else pt, dev)
    sn, st_ = (c, n * c) if transposed else (t * c, c)
    sz = None if sizes is None else PoisonedI32(torch.tensor(sizes, dtype=torch.int32), dev)
    ids, offs, counts = PoisonedI32((n, t), dev), PoisonedI32((n, t), dev), PoisonedI32((n,), dev)
    am = PoisonedI32((n, t), dev) if want_argmax else None
    st = _lib.load().ds2_greedy_decode(p.ptr, n, t, c, sn, st_, None if sz is None else sz.ptr, blank,
                                       ids.ptr, offs.ptr, counts.ptr, None if am is None else am.ptr,
                                       None)
    _lib.check(st, "ds2_greedy_decode")
    torch.cuda.synchronize()
    intact = ids.intact() and offs.intact() and counts.intact() and (am is None or am.intact())
    return ids.read(), offs.read(), counts.read(), None if am is None else am.read(), intact


# ------------------------------------------------------------------------------------------
# edit distance

ED_MAXC, ED_MAXW = 2048, 1024       # csrc/ctc.hip: non-space ids and words per sequence
ED_REG_COLS = 256                   # reference lengths below it run the register DP
SPACE = 28


def ed_words(ids, space=SPACE):
    out, cur = [], []
    for v in ids:
        if v == space:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(v)
    if cur:
        out.append(tuple(cur))
    return out


def ed_ref(a, b, space=SPACE):
    """[word distance, char distance, max(#reference words, 1), max(#reference chars, 1)] of
    decoded ids a against reference ids b: ds2amd.decoder._levenshtein on exact word ids and on
    the space-stripped ids."""
    wa, wb = ed_words(a, space), ed_words(b, space)
    wid = {}
    ia, ib = [wid.setdefault(w, len(wid)) for w in wa], [wid.setdefault(w, len(wid)) for w in wb]
    ca, cb = [v for v in a if v != space], [v for v in b if v != space]
    return [_levenshtein(ia, ib), _levenshtein(ca, cb), max(len(wb), 1), max(len(cb), 1)]


def ed_delete(a, k, rng):
    """a with k of its ids deleted: the lengths differ by k and k deletions suffice, so the
    distance is exactly k."""
    drop = set(rng.choice(len(a), k, replace=False).tolist())
    return [v for i, v in enumerate(a) if i not in drop]


def ed_delete_at(a, positions):
    """a without the ids at `positions`.  Scored against a as the reference, the id at position
    p is an insertion at DP column p + 1: p = 64 c - 1 puts it in the first lane of a 64-column
    chunk, where the row's running minimum arrives only through the carry between chunks."""
    drop = set(positions)
    assert len(drop) == len(positions) and all(0 <= p < len(a) for p in drop)
    return [v for i, v in enumerate(a) if i not in drop]


def ed_distinct(n, first=100):
    """n distinct ids (none the space): the optimal alignment against a copy with deletions is
    the only one."""
    assert first > SPACE
    return list(range(first, first + n))


def ed_replace(a, k, rng, new):
    """a with k positions replaced by an id a does not contain: each of the k new ids costs an
    edit and k substitutions suffice, so the distance is exactly k."""
    assert new not in a
    out = list(a)
    for i in rng.choice(len(a), k, replace=False).tolist():
        out[i] = new
    return out


def ed_with_spaces(ids, every, space=SPACE, limit=None):
    """A space after every `every` ids (none at the end), `limit` spaces at the most."""
    out, spaces = [], 0
    for i, v in enumerate(ids):
        if i and i % every == 0 and (limit is None or spaces < limit):
            out.append(space)
            spaces += 1
        out.append(v)
    return out


def run_edit(a_rows, b_rows, dev, space=SPACE, slack=37, err=None):
    """ds2_edit_distance on a [n][a_stride] with a_stride = the longest row + slack and -1
    behind every row, b flat.  err: a held_i32 word to reuse, else a fresh zeroed one.  Returns
    (out [n][4] on the CPU, the err word's value, the err word, canaries intact)."""
    n = len(a_rows)
    stride = max(len(r) for r in a_rows) + slack
    a = torch.full((n, stride), -1, dtype=torch.int32)
    for i, r in enumerate(a_rows):
        a[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    lens = lambda rows: torch.tensor([len(r) for r in rows], dtype=torch.int32)
    b = torch.tensor([v for r in b_rows for v in r] or [0], dtype=torch.int32)
    bl = lens(b_rows)
    ops_ = [PoisonedI32(v, dev) for v in (a, lens(a_rows), b, (torch.cumsum(bl, 0) - bl).to(torch.int32), bl)]
    out = PoisonedI32((n, 4), dev)
    err = held_i32(torch.zeros(1), dev) if err is None else err
    st = _lib.load().ds2_edit_distance(ops_[0].ptr, stride, ops_[1].ptr, ops_[2].ptr, ops_[3].ptr,
                                       ops_[4].ptr, n, space, out.ptr, err.ptr, None)
    _lib.check(st, "ds2_edit_distance")
    torch.cuda.synchronize()
    return out.read(), int(err.read().item()), err, out.intact() and err.intact()


# ------------------------------------------------------------------------------------------
# reductions and guards

COL_CHUNKS = 64                     # csrc/misc.hip kColChunks: row chunks = clamp(rows / 64, 1, 64)
GRID_CAP, BLOCK = 2048, 256         # grid_for: the grid-stride kernels' first trip covers 2048 x 256
COLSUM_ROWS = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4096, 4097)
# (cols, ld, off, the partial kernel the entry point selects)
COLSUM_FORMS = ((4, 4, 0, "vector"), (256, 260, 0, "vector"), (260, 264, 0, "vector"),
                (5, 7, 0, "scalar"), (260, 261, 0, "scalar"), (256, 260, 1, "scalar"))
DIRSUM_SHAPES = ((7, 1, 5), (7, 2, 5), (33, 2, 64), (2049, 2, 257))
NORM_NUMELS = (0, 1, 3, 4, 5, 6, 1023, 2 * GRID_CAP * BLOCK * 4 + 3)
GUARD_NUMEL = GRID_CAP * BLOCK + 5


def colsum_chunks(rows):
    return min(max(rows // 64, 1), COL_CHUNKS)


def colsum_is_vector(cols, ld, addr):
    """ds2_colsum's selection: float4 loads need ld, cols multiples of 4 and a 16-byte address."""
    return ld % 4 == 0 and cols % 4 == 0 and addr % 16 == 0


def colsum_inputs(rows, cols, ld, off, integer=False):
    """(storage [rows][ld]: the data in columns off .. off + cols, NaN in the others; out0)."""
    g = torch.Generator().manual_seed(7919 * rows + 31 * cols + ld + off)
    if integer:
        data = torch.randint(-8, 9, (rows, cols), generator=g).double()
        out0 = torch.randint(-8, 9, (cols,), generator=g).double()
    else:
        data = torch.randn(rows, cols, generator=g, dtype=torch.float64).float().double()
        out0 = torch.randn(cols, generator=g, dtype=torch.float64).float().double()
    storage = torch.full((rows, ld), float("nan"), dtype=torch.float64)
    storage[:, off:off + cols] = data
    return storage, data, out0


def colsum_ref(data, out0, accumulate):
    """(reference, bound 2).  The kernels sum in fp64 -- each of the rows additions rounds to
    2^-53 of a partial sum that sum |x| bounds -- then round once to float32 and, under
    accumulate, once more after adding out0."""
    rows = data.shape[0]
    s = data.sum(0)
    ref = s + out0 if accumulate else s
    bound = 2 * U * (ref.abs() + (out0.abs() if accumulate else 0)) + rows * 2.0 ** -53 * data.abs().sum(0)
    return ref, bound


def run_colsum(storage, rows, cols, ld, off, out0, accumulate, dev, ws_fill=0xFF):
    """ds2_colsum on the data inside NaN, out holding out0 between canaries, exactly the query's
    workspace.  Returns (out on the CPU, the address of x, canaries intact)."""
    x = Poisoned(storage if rows else torch.zeros(0), dev)
    out = held(out0, dev)
    ws = Workspace(_lib.size("ds2_colsum_workspace_size", rows, cols), dev, ws_fill)
    addr = x.ptr + 4 * off
    st = _lib.load().ds2_colsum(addr, rows, cols, ld, out.ptr, accumulate, ws.ptr, ws.nbytes, None)
    _lib.check(st, "ds2_colsum")
    torch.cuda.synchronize()
    return out.read(), addr, out.intact() and ws.intact()


def norm_input(numel):
    g = torch.Generator().manual_seed(numel % 100003 + 1)
    return torch.randn(numel, generator=g)


def run_grad_norm(x, dev, ws_fill=0xFF):
    """ds2_grad_norm on x followed by NaN.  Returns (the norm as a float, canaries intact)."""
    xp = Poisoned(x, dev)
    out = Poisoned((1,), dev)
    ws = Workspace(_lib.size("ds2_optim_workspace_size", x.numel()), dev, ws_fill)
    st = _lib.load().ds2_grad_norm(xp.ptr, x.numel(), out.ptr, ws.ptr, ws.nbytes, None)
    _lib.check(st, "ds2_grad_norm")
    torch.cuda.synchronize()
    return out.read().item(), out.intact() and ws.intact()
