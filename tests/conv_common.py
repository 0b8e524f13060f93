"""Helpers of the Conv2d contract tests (test_gpu_conv_contract.py, test_conv_contract_cpu.py):
the shape table with the rung every case is there for, float64 references cached per shape,
operands placed inside larger poisoned allocations, and the three C entry points called
directly with a workspace of exactly the plan's size."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

from ds2amd import _lib, ops

from test_conv_plan_cpu import SETTINGS, set_env, rung_name  # noqa: F401  (re-exported)

CANARY = 0x5CA1AB1E     # the word every element of an output allocation outside the tensor holds
LEAD16 = 68             # floats before a tensor: 272 bytes, 16-byte aligned, not 256-byte aligned
LEAD4 = 69              # 276 bytes: 4-byte aligned only
TAIL = 1024             # floats after it
WS_LEAD = 256           # bytes before the workspace (allocations are >= 256-byte aligned)
WS_TAIL = 4096          # bytes after it
DIRS = ("fwd", "dgrad", "wgrad")

# id -> ((n, ci, h, w, co, kh, kw, sh, sw, ph, pw), {setting: (fwd, dgrad, wgrad rung or None)}).
# None: the case is not there for that direction under that setting (the rung it takes there
# is another case's).  "default" names all three: the poison test runs every direction there.
Case = collections.namedtuple("Case", "cfg rungs")


def _j(kw, a):
    return Case((2, 1, 20, 70, 8, 5, kw, 2, 2, 2, kw // 2),
                {"default": (f"fwd_c1:{a}", "dg_gemm", "wg_patch:2:2")})


CASES = {
    # conv2's taps with 33 -> 33 channels (two channel blocks with one channel in the second, on
    # both the output side M and the loop side L), 258 = 256 + 2 columns, 9 = 8 + 1 output rows
    # (a lone row in the two-row pairing; dgrad class rows 9 + 8)
    "A": Case((2, 33, 17, 258, 33, 21, 11, 2, 1, 10, 5), {
        "default": ("fwd_h3_2r", "dg_h3_2r", "wg_patch:2:1"),
        "x6": ("fwd_x6_db", "dg_x6_q", None),
        "fp32": ("fwd_patch", "dg_patch", None),
        "one_row": ("fwd_h3_1r", "dg_h3_q", None),
        "one_row_noflush": (None, "dg_h3_q_noflush", None)}),
    # sliding-window wgrad, 35 = 32 + 3 columns, 3 -> 5 channels; sample planes of 1785 and 1395
    # floats: samples 1 and 2 start 4-byte aligned only (the scalar branch of the fp16x3
    # sample-maximum kernel)
    "B": Case((3, 3, 17, 35, 5, 21, 11, 2, 1, 10, 5), {
        "default": ("fwd_h3_2r", "dg_h3_2r", "wg_h3_sw32"),
        "x6": (None, None, "wg_x6_sw"),
        "w64": (None, None, "wg_h3_sw64")}),
    # the sliding window at row stride 1, 67 = 64 + 3 columns
    "C": Case((3, 5, 17, 67, 7, 21, 11, 1, 1, 10, 5), {
        "default": ("fwd_h3_1r", "dg_x6", "wg_h3_sw32"),
        "w64": (None, None, "wg_h3_sw64")}),
    # dgrad over three stride classes; per-row re-staging wgrad
    "D": Case((3, 5, 17, 67, 7, 7, 11, 3, 1, 3, 5), {
        "default": ("fwd_x6", "dg_h3_2r", "wg_x6_row")}),
    # two column tiles, 33 input channels
    "E": Case((2, 33, 40, 258, 5, 31, 11, 2, 1, 15, 5), {
        "default": ("fwd_gemm", "dg_x6_26", "wg_patch:4:1")}),
    # 33 loop channels
    "F": Case((2, 33, 20, 258, 3, 15, 5, 1, 1, 7, 2), {
        "default": ("fwd_x6", "dg_x6", "wg_patch:2:1")}),
    # the patch rungs by shape (13 kernel columns), 131 = 128 + 3 columns, 9 = 2 * 4 + 1 rows
    "G": Case((2, 33, 9, 131, 33, 5, 13, 1, 1, 2, 6), {
        "default": ("fwd_patch", "dg_patch", "wg_patch:2:1")}),
    # width stride 2
    "H": Case((2, 33, 11, 131, 33, 3, 3, 2, 2, 1, 1), {
        "default": ("fwd_gemm", "dg_gemm", "wg_patch:2:2")}),
    # width stride 3
    "I": Case((2, 5, 17, 66, 33, 5, 5, 1, 3, 2, 2), {
        "default": ("fwd_gemm", "dg_gemm", "wg_gemm")}),
    # the single-channel patch forward: every KWH instance, odd and even kw (an even kw has no
    # padded tap column)
    "J3": _j(3, 2), "J4": _j(4, 2), "J5": _j(5, 3), "J6": _j(6, 3), "J7": _j(7, 4),
    "J8": _j(8, 4), "J9": _j(9, 5), "J10": _j(10, 5),
    # ... with two column tiles (wo 130 = 128 + 2) and ho 10 = 2 * 4 + 2
    "J2": Case((2, 1, 19, 259, 8, 5, 7, 2, 2, 2, 3), {
        "default": ("fwd_c1:4", "dg_gemm", "wg_patch:2:2")}),
    # 287 taps at width stride 2
    "K": Case((2, 1, 50, 70, 8, 41, 7, 2, 2, 20, 3), {
        "default": ("fwd_c1:4", "dg_gemm", "wg_patch:4:2")}),
    # kh < sh: a stride class without taps
    "L1": Case((2, 4, 9, 20, 8, 1, 3, 2, 1, 0, 1), {
        "default": ("fwd_x6", "dg_h3_2r", "wg_patch:2:1"),
        "fp32": ("fwd_patch", "dg_patch", None)}),
    # ... and kw < sw: columns without a tap
    "L2": Case((2, 4, 9, 20, 8, 2, 2, 3, 3, 0, 0), {
        "default": ("fwd_gemm", "dg_gemm", "wg_gemm")}),
}

_S1 = {"default": ("fwd_h3_2r", None, None), "x6": ("fwd_x6_db", None, None),
       "fp32": ("fwd_patch", None, None), "one_row": ("fwd_h3_1r", None, None)}
# the windows StreamingSession feeds the two convolutions: time padding 0, wo 1 and 2
STREAMING = {
    "S1a": Case((2, 32, 81, 11, 32, 21, 11, 2, 1, 10, 0), _S1),
    "S1b": Case((2, 32, 81, 12, 32, 21, 11, 2, 1, 10, 0), _S1),
    "S2a": Case((2, 1, 161, 11, 32, 41, 11, 2, 2, 20, 0), {"default": ("fwd_c1:6", None, None)}),
    "S2b": Case((2, 1, 161, 13, 32, 41, 11, 2, 2, 20, 0), {"default": ("fwd_c1:6", None, None)}),
}
ALL_CASES = {**CASES, **STREAMING}


def case_settings(cases=None):
    """[(case id, setting)] of the table, in its order."""
    return [(c, s) for c, case in (cases or CASES).items() for s in case.rungs]


def table_rungs():
    """Every rung name the table claims."""
    return {r for case in ALL_CASES.values() for rungs in case.rungs.values() for r in rungs if r}


def with_n(cfg, n):
    return (n,) + tuple(cfg[1:])


def out_hw(cfg):
    n, ci, h, w, co, kh, kw, sh, sw, ph, pw = cfg
    return ops.conv_out_shape(h, w, kh, kw, sh, sw, ph, pw)


def plans(cfg):
    """{direction: the library's plan} under the current environment."""
    n, ci, h, w, co, kh, kw, sh, sw, ph, pw = cfg
    return {d: ops.conv2d_plan(d, (n, ci, h, w), (co, ci, kh, kw), (sh, sw), (ph, pw))
            for d in DIRS}


def assert_rungs(cfg, want):
    """The planned rung of every direction `want` names; returns the plans."""
    p = plans(cfg)
    for d, r in zip(DIRS, want):
        assert r is None or rung_name(p[d]) == r, (cfg, d, rung_name(p[d]), r)
    return p


Ref = collections.namedtuple("Ref", "x w b dy y dx dw db")


@functools.lru_cache(maxsize=None)
def ref64(cfg):
    """Inputs (values that float32 holds exactly) and the float64 results on the CPU, seeded
    from the shape.  Shared by every setting and test: never modify the tensors."""
    n, ci, h, w, co, kh, kw, sh, sw, ph, pw = cfg
    g = torch.Generator().manual_seed(zlib.crc32(",".join(map(str, cfg)).encode()))
    ho, wo = out_hw(cfg)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()

    x = rnd(n, ci, h, w)
    wt = (rnd(co, ci, kh, kw) * 0.1).float().double()
    b = rnd(co)
    dy = rnd(n, co, ho, wo)
    y = F.conv2d(x, wt, b, stride=(sh, sw), padding=(ph, pw))
    dx = torch.nn.grad.conv2d_input(x.shape, wt, dy, stride=(sh, sw), padding=(ph, pw))
    dw = torch.nn.grad.conv2d_weight(x, wt.shape, dy, stride=(sh, sw), padding=(ph, pw))
    return Ref(x, wt, b, dy, y, dx, dw, dy.sum(dim=(0, 2, 3)))


class Poisoned:
    """A float32 tensor inside a larger live device allocation, `lead` floats after its start
    and TAIL floats before its end.  An input (a CPU tensor is given) has NaN everywhere else;
    an output (a shape is given) has the canary word everywhere else and NaN inside, so an
    element the kernel never writes shows.  All poison is live memory: a stray access cannot
    fault."""

    def __init__(self, data_or_shape, dev, lead=LEAD16):
        is_input = isinstance(data_or_shape, torch.Tensor)
        self.shape = tuple(data_or_shape.shape) if is_input else tuple(data_or_shape)
        self.numel = 1
        for s in self.shape:
            self.numel *= s
        self.lead = lead
        total = lead + self.numel + TAIL
        if is_input:
            host = torch.full((total,), float("nan"), dtype=torch.float32)
            host[lead:lead + self.numel] = data_or_shape.reshape(-1).float()
        else:
            host = torch.full((total,), CANARY, dtype=torch.int32).view(torch.float32)
            host[lead:lead + self.numel] = float("nan")
        self.buf = host.to(dev)
        assert self.buf.data_ptr() % 256 == 0
        assert self.ptr % 4 == 0 and self.ptr % 256 != 0 and (self.ptr % 16 == 0) == (lead % 4 == 0)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lead

    @property
    def view(self):
        """The tensor itself, on the device (shares the allocation)."""
        return self.buf[self.lead:self.lead + self.numel].view(self.shape)

    def read(self):
        return self.view.cpu()

    def intact(self):
        """Every word of an output allocation outside the tensor still holds the canary."""
        w = self.buf.view(torch.int32)
        return bool((w[:self.lead] == CANARY).all().item() and
                    (w[self.lead + self.numel:] == CANARY).all().item())


class Workspace:
    """Exactly `nbytes` bytes, 256-byte aligned, every byte `fill`, inside an allocation whose
    remainder holds the canary."""

    def __init__(self, nbytes, dev, fill=0xFF):
        self.nbytes = int(nbytes)
        total = WS_LEAD + (self.nbytes + 3) // 4 * 4 + WS_TAIL
        host = torch.full((total // 4,), CANARY, dtype=torch.int32).view(torch.uint8)
        host[WS_LEAD:WS_LEAD + self.nbytes] = fill
        end = WS_LEAD + self.nbytes
        self.before = (host[:WS_LEAD].clone(), host[end:].clone())
        self.buf = host.to(dev)
        assert self.buf.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + WS_LEAD

    def intact(self):
        end = WS_LEAD + self.nbytes
        return (torch.equal(self.buf[:WS_LEAD].cpu(), self.before[0]) and
                torch.equal(self.buf[end:].cpu(), self.before[1]))


def _dims(cfg):
    return tuple(int(v) for v in cfg)


def _plan(direction, cfg):
    n, ci, h, w, co, kh, kw, sh, sw, ph, pw = cfg
    return ops.conv2d_plan(direction, (n, ci, h, w), (co, ci, kh, kw), (sh, sw), (ph, pw))


def _lens(out_lens, dev):
    return None if out_lens is None else torch.tensor(out_lens, dtype=torch.int32, device=dev)


def run_fwd(cfg, x, w, b, dev, out_lens=None, lead=LEAD16, ws_fill=0xFF):
    """ds2_conv2d_fwd on Poisoned x, w, b (b None: no bias).  Returns (y on the CPU, the plan,
    whether every canary around y and behind the workspace is intact)."""
    n, ci, h, wi, co = cfg[:5]
    plan = _plan("fwd", cfg)
    y = Poisoned((n, co) + out_hw(cfg), dev, lead)
    ws = Workspace(plan.ws_bytes, dev, ws_fill)
    lens = _lens(out_lens, dev)
    st = _lib.load().ds2_conv2d_fwd(x.ptr, w.ptr, None if b is None else b.ptr, y.ptr, *_dims(cfg),
                                    None if lens is None else lens.data_ptr(), ws.ptr,
                                    plan.ws_bytes, None)
    _lib.check(st, "ds2_conv2d_fwd")
    torch.cuda.synchronize()
    return y.read(), plan, y.intact() and ws.intact()


def run_dgrad(cfg, dy, w, dev, lead=LEAD16, ws_fill=0xFF):
    """ds2_conv2d_dgrad on Poisoned dy, w.  Returns (dx on the CPU, plan, canaries intact)."""
    n, ci, h, wi = cfg[:4]
    plan = _plan("dgrad", cfg)
    dx = Poisoned((n, ci, h, wi), dev, lead)
    ws = Workspace(plan.ws_bytes, dev, ws_fill)
    st = _lib.load().ds2_conv2d_dgrad(dy.ptr, w.ptr, dx.ptr, *_dims(cfg), ws.ptr, plan.ws_bytes,
                                      None)
    _lib.check(st, "ds2_conv2d_dgrad")
    torch.cuda.synchronize()
    return dx.read(), plan, dx.intact() and ws.intact()


def run_wgrad(cfg, dy, x, dev, with_bias=True, lead=LEAD16, ws_fill=0xFF):
    """ds2_conv2d_wgrad on Poisoned dy, x.  Returns ((dw, db or None) on the CPU, plan, canaries
    intact)."""
    n, ci, h, wi, co, kh, kw = cfg[:7]
    plan = _plan("wgrad", cfg)
    dw = Poisoned((co, ci, kh, kw), dev, lead)
    db = Poisoned((co,), dev, lead) if with_bias else None
    ws = Workspace(plan.ws_bytes, dev, ws_fill)
    st = _lib.load().ds2_conv2d_wgrad(dy.ptr, x.ptr, dw.ptr, None if db is None else db.ptr,
                                      *_dims(cfg), ws.ptr, plan.ws_bytes, None)
    _lib.check(st, "ds2_conv2d_wgrad")
    torch.cuda.synchronize()
    ok = dw.intact() and ws.intact() and (db is None or db.intact())
    return (dw.read(), None if db is None else db.read()), plan, ok


def close(got, ref, rel=1e-5, name=""):
    """test_gpu_ops._close's bound, max |err| <= rel * max |ref|; prints the error as a fraction
    of the bound before it asserts."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    print(f"CONV_CONTRACT {name}: err / bound = {err / (rel * scale):.3f}")
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"
