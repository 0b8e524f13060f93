"""Helpers of the Conv1d contract tests (test_gpu_conv1d_contract.py,
test_conv1d_contract_cpu.py): the shape table with the path every case takes in each direction,
float64 references and magnitude references cached per shape, and the three C entry points
called directly on operands inside poisoned allocations (conv_common.Poisoned) with a workspace
of exactly the size query's bytes.

Layouts: the references are torch's ([N, C, T]); the device holds time-major activations
([T, N, C]).  run_* take Poisoned operands in the device layout (tnc()) and return results in
the reference's layout."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

from ds2amd import _lib, ops

from conv_common import CANARY, LEAD4, LEAD16, Poisoned, Workspace  # noqa: F401  (re-exported)

DIRS = ("fwd", "dgrad", "wgrad")
SETTINGS = ("default", "general")     # general: DS2_CONV1D=0
VEC, SCALAR, H3, GEN, GEMM = "igemm_vec", "igemm_scalar", "wgrad_h3", "general", "gemm"

# id -> ((T, N, Cin, Cout, k, s, p), (forward, dgrad, wgrad path under the default environment)).
# Under DS2_CONV1D=0 every direction of every case is "general".
Case = collections.namedtuple("Case", "cfg paths")
CASES = {
    # the prolog with a bias: Cin % 4 != 0 (scalar loader), 78 stages, the s = 2 dgrad on the
    # general kernel, wgrad's NN = 2093 = 16 * 128 + 45 columns, Cout = 16
    "A": Case((37, 3, 161, 16, 13, 2, 6), (SCALAR, GEN, H3)),
    # Cin = 36: the second channel chunk holds 4 channels; Cout = 130 = 128 + 2; M = 135 =
    # 128 + 7; 10 stages; dgrad loops over 130 channels (scalar loader, 160 padded, 25 stages);
    # wgrad has two row tiles and NN = 180
    "B": Case((45, 3, 36, 130, 5, 1, 2), (VEC, SCALAR, H3)),
    # Cin = 20: a float4 on the channel edge; even k; p = k - 1: T_out = 22 > T (the maxima
    # buffer is sized by T_out), flipped padding 0
    "C": Case((19, 2, 20, 24, 4, 1, 3), (VEC, VEC, H3)),
    # the thresholds exactly (16, 16, k Cin = 64); p = 0, flipped padding 3; 4 stages: only the
    # final flush
    "D": Case((19, 2, 16, 16, 4, 1, 0), (VEC, VEC, H3)),
    # Cin = 15: general by shape; K = 75 is no multiple of 16
    "D1": Case((19, 2, 15, 16, 5, 1, 2), (GEN, GEN, GEN)),
    # k Cin = 48 < 64
    "D2": Case((19, 2, 16, 16, 3, 1, 1), (GEN, GEN, H3)),
    # k Cout = 48 declines dgrad only
    "E": Case((23, 2, 64, 16, 3, 1, 1), (VEC, GEN, H3)),
    # k = 1 but no GEMM: 2 stages; the 10 odd input rows are reached by no tap
    "F1": Case((21, 3, 64, 32, 1, 2, 0), (VEC, GEN, H3)),
    # output rows 0 and 22 are padding only; p > k - 1 declines dgrad
    "F2": Case((21, 3, 64, 32, 1, 1, 1), (VEC, GEN, H3)),
    # s > k, (T - k) % s = 2: 14 input rows reached by no tap; wgrad at s = 3
    "G": Case((40, 2, 32, 32, 2, 3, 0), (VEC, GEN, H3)),
    # p > k: output rows 0, 1, 13, 14 are padding only
    "H": Case((9, 2, 32, 32, 3, 1, 4), (VEC, GEN, H3)),
    # 903 rows (7 tiles + 7); wgrad: 4 slabs of 256, the last 135 = 4 stages + 7; N = 3 wraps
    # five times inside 16 rows
    "I": Case((301, 3, 32, 32, 13, 1, 6), (VEC, VEC, H3)),
    # N = 1: wgrad's (t, n) counter wraps at every row
    "J1": Case((70, 1, 32, 32, 13, 1, 6), (VEC, VEC, H3)),
    # N = 37 > 32: a wgrad stage lies inside one time step
    "J2": Case((5, 37, 32, 32, 3, 1, 1), (VEC, VEC, H3)),
    # 9 stages: one flush + 1
    "K": Case((20, 2, 96, 16, 3, 1, 1), (VEC, GEN, H3)),
    # M = 128 exactly
    "L": Case((64, 2, 32, 16, 5, 1, 2), (VEC, VEC, H3)),
    # the re-laid weights are 2 158 592 floats (2 285 568 flipped) and dw is 2 158 592, past the
    # 2 097 152 one pass of a grid-stride kernel covers; Cout has three tiles; 248 stages
    "R": Case((8, 1, 256, 272, 31, 1, 15), (VEC, VEC, H3)),
    # the fc layer: a GEMM on all three
    "P1": Case((19, 3, 24, 30, 1, 1, 0), (GEMM, GEMM, GEMM)),
}


def set_env(monkeypatch, setting):
    assert setting in SETTINGS
    if setting == "general":
        monkeypatch.setenv("DS2_CONV1D", "0")
    else:
        monkeypatch.delenv("DS2_CONV1D", raising=False)


def want_paths(case, setting):
    return CASES[case].paths if setting == "default" else (GEN, GEN, GEN)


def case_settings(cases=None):
    return [(c, s) for c in (cases or CASES) for s in SETTINGS]


def with_n(cfg, n):
    return (cfg[0], n) + tuple(cfg[2:])


def out_len(cfg):
    t, n, ci, co, k, s, p = cfg
    return (t + 2 * p - k) // s + 1


def plan(direction, cfg, addr=0, amax_given=False):
    t, n, ci, co, k, s, p = cfg
    return ops.conv1d_plan(direction, (t, n, ci), (co, ci, k), s, p, addr=addr,
                           amax_given=amax_given)


def plans(cfg, addr=0):
    """{direction: the library's plan} under the current environment."""
    return {d: plan(d, cfg, addr) for d in DIRS}


def assert_paths(cfg, want, addr=0):
    """The planned path of every direction; returns the plans."""
    p = plans(cfg, addr)
    for d, w in zip(DIRS, want):
        assert w is None or p[d].path == w, (cfg, d, p[d].path, w)
    return p


def query(direction, cfg):
    """The workspace-size query that serves the direction."""
    name = "ds2_conv1d_wgrad_workspace_size" if direction == "wgrad" else "ds2_conv1d_workspace_size"
    return _lib.size(name, *cfg)


def tnc(x_nct):
    return x_nct.permute(2, 0, 1).contiguous()


def nct(x_tnc):
    return x_tnc.permute(1, 2, 0).contiguous()


# x, w, b, dy and the float64 results; *_mag: the same sums over absolute values (the scale of
# a componentwise bound); cpu32: float32 CPU torch's componentwise error ratio per result
Ref = collections.namedtuple("Ref", "x w b dy y dx dw db y_mag dx_mag dw_mag db_mag cpu32")


def mags(x, w, b, dy, s, p):
    """|w| conv |x| + |b|, conv1d_input(|w|, |dy|), conv1d_weight(|x|, |dy|), sum |dy|."""
    return (F.conv1d(x.abs(), w.abs(), None if b is None else b.abs(), stride=s, padding=p),
            torch.nn.grad.conv1d_input(x.shape, w.abs(), dy.abs(), stride=s, padding=p),
            torch.nn.grad.conv1d_weight(x.abs(), w.shape, dy.abs(), stride=s, padding=p),
            dy.abs().sum((0, 2)))


def results(x, w, b, dy, s, p):
    return (F.conv1d(x, w, b, stride=s, padding=p),
            torch.nn.grad.conv1d_input(x.shape, w, dy, stride=s, padding=p),
            torch.nn.grad.conv1d_weight(x, w.shape, dy, stride=s, padding=p),
            dy.sum((0, 2)))


@functools.lru_cache(maxsize=None)
def ref64(cfg):
    """Inputs (values that float32 holds exactly, w scaled by 0.1, always a bias) and the float64
    results on the CPU, seeded from the shape.  Shared by every setting and test: never modify
    the tensors."""
    t, n, ci, co, k, s, p = cfg
    g = torch.Generator().manual_seed(zlib.crc32(",".join(map(str, cfg)).encode()))

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()

    x = rnd(n, ci, t)
    w = (rnd(co, ci, k) * 0.1).float().double()
    b = rnd(co)
    dy = rnd(n, co, out_len(cfg))
    res = results(x, w, b, dy, s, p)
    mag = mags(x, w, b, dy, s, p)
    r32 = results(x.float(), w.float(), b.float(), dy.float(), s, p)
    cpu32 = tuple(((a.double() - r).abs() / m.clamp_min(1e-300)).max().item()
                  for a, r, m in zip(r32, res, mag))
    return Ref(x, w, b, dy, *res, *mag, dict(zip(("y", "dx", "dw", "db"), cpu32)))


def _ws(direction, cfg, dev, ws_bytes, fill):
    return Workspace(query(direction, cfg) if ws_bytes is None else ws_bytes, dev, fill)


def run_fwd(cfg, x, w, b, dev, lead=LEAD16, ws_fill=0xFF, ws_bytes=None, amax=None):
    """ds2_conv1d_fwd_amax on Poisoned x [T, N, Cin], w, b (None: no bias); amax: a device
    pointer to x's row maxima or None.  Returns (y [N, Cout, T_out] on the CPU, the plan, whether
    every canary around y and around the workspace is intact)."""
    t, n, ci, co = cfg[:4]
    pl = plan("fwd", cfg, x.ptr, amax is not None)
    y = Poisoned((out_len(cfg), n, co), dev, lead)
    ws = _ws("fwd", cfg, dev, ws_bytes, ws_fill)
    st = _lib.load().ds2_conv1d_fwd_amax(x.ptr, w.ptr, None if b is None else b.ptr, y.ptr, *cfg,
                                         amax, ws.ptr, ws.nbytes, None)
    _lib.check(st, "ds2_conv1d_fwd_amax")
    torch.cuda.synchronize()
    return nct(y.read()), pl, y.intact() and ws.intact()


def run_dgrad(cfg, dy, w, dev, lead=LEAD16, ws_fill=0xFF, ws_bytes=None):
    """ds2_conv1d_dgrad on Poisoned dy [T_out, N, Cout], w.  Returns (dx [N, Cin, T] on the CPU,
    plan, canaries intact)."""
    t, n, ci = cfg[:3]
    pl = plan("dgrad", cfg, dy.ptr)
    dx = Poisoned((t, n, ci), dev, lead)
    ws = _ws("dgrad", cfg, dev, ws_bytes, ws_fill)
    st = _lib.load().ds2_conv1d_dgrad(dy.ptr, w.ptr, dx.ptr, *cfg, ws.ptr, ws.nbytes, None)
    _lib.check(st, "ds2_conv1d_dgrad")
    torch.cuda.synchronize()
    return nct(dx.read()), pl, dx.intact() and ws.intact()


def run_wgrad(cfg, dy, x, dev, with_bias=True, lead=LEAD16, ws_fill=0xFF, ws_bytes=None, amax=None):
    """ds2_conv1d_wgrad_amax on Poisoned dy, x; amax: a device pointer to x's column maxima or
    None.  Returns ((dw, db or None) on the CPU, plan, canaries intact)."""
    t, n, ci, co, k = cfg[:5]
    pl = plan("wgrad", cfg, 0, amax is not None)
    dw = Poisoned((co, ci, k), dev, lead)
    db = Poisoned((co,), dev, lead) if with_bias else None
    ws = _ws("wgrad", cfg, dev, ws_bytes, ws_fill)
    st = _lib.load().ds2_conv1d_wgrad_amax(dy.ptr, x.ptr, dw.ptr, None if db is None else db.ptr,
                                           *cfg, amax, ws.ptr, ws.nbytes, None)
    _lib.check(st, "ds2_conv1d_wgrad_amax")
    torch.cuda.synchronize()
    ok = dw.intact() and ws.intact() and (db is None or db.intact())
    return (dw.read(), None if db is None else db.read()), pl, ok


GLOBAL_REL = 1e-5    # the project's conv bound: max |err| <= 1e-5 max |ref|
COMP_REL = 2e-6      # |err| <= 2e-6 mag elementwise: 8 x what float32 CPU torch needs (2.5e-7)


def close(got, ref, mag, name, cpu32=None):
    """Both bounds, and got == 0 wherever mag == 0 (every term of the sum is an exact zero).
    Prints the errors as fractions of the bounds before it asserts; cpu32: float32 CPU torch's
    componentwise ratio on the same inputs, printed beside them."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    assert got.shape == ref.shape == mag.shape, (name, got.shape, ref.shape, mag.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).abs()
    scale = max(ref.abs().max().item(), 1e-30)
    g = err.max().item() / (GLOBAL_REL * scale)
    zero = mag == 0
    comp = (err / mag.clamp_min(1e-300))[~zero]
    c = (comp.max().item() if comp.numel() else 0.0) / COMP_REL
    tail = "" if cpu32 is None else f"  cpu float32 componentwise {cpu32:.2e}"
    print(f"CONV1D_CONTRACT {name}: global err / bound = {g:.3f}  "
          f"componentwise err / bound = {c:.3f}{tail}")
    assert g <= 1, f"{name}: max err {err.max().item():.3e} > {GLOBAL_REL:.0e} * {scale:.3e}"
    assert c <= 1, f"{name}: componentwise error {c * COMP_REL:.3e} of the magnitude > {COMP_REL:.0e}"
    assert (got[zero] == 0).all(), f"{name}: a sum of exact zeros is not exactly 0"
