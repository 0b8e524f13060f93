"""A/B timing of the GRU recurrence variants at the bench shape (T=501, N=32, H=800,
bidirectional), alternating in one process: the bf16x6 kernels vs the fp32-MFMA ones, the
same-XCD groups vs the interleaved layout, and poll-knob sweeps (DS2_RNN_TUNE) -- selected
through the environment switches the library reads at every call."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "deepspeech.pytorch_amd"))

# `libs name=path name=path ...`: builds of the library against each other (say the parent
# commit's and the tree's), alternating AB_ROUNDS times in one call, one fresh child process per
# turn (DS2_LIB_PATH).  Every child runs the product calls (forward; backward with bias
# gradients, column maxima and the row-maximum partials) at the bench shape and at the shapes
# of tests/test_gpu_gru_xl_instances.py, times them and prints a SHA-256 per output; the parent
# prints the per-launch times and whether every output is bit-equal across the builds.
LIB_SHAPES = [(501, 32, 800, 2), (27, 9, 288, 2), (29, 8, 416, 1), (31, 12, 544, 2), (33, 5, 672, 1)]
if len(sys.argv) > 1 and sys.argv[1] == "libs":
    import json
    import subprocess
    libs = [a.split("=", 1) for a in sys.argv[2:]]
    seen, equal = {}, True
    for r in range(int(os.environ.get("AB_ROUNDS", "3"))):
        for name, path in libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "libchild"],
                                 env=dict(os.environ, DS2_LIB_PATH=os.path.abspath(path)),
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(f"{name}: exit {out.returncode}\n{out.stdout}\n{out.stderr}")
            for line in out.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                rec = json.loads(line)
                ref = seen.setdefault(rec["shape"], rec["sha"])
                diff = [k for k in ref if ref[k] != rec["sha"][k]]
                equal = equal and not diff
                print(f"{name}#{r} {rec['shape']:>16s} fwd {rec['fwd_us']:8.1f} us  bwd "
                      f"{rec['bwd_us']:8.1f} us  " + ("bit-equal" if not diff else f"DIFFERS {diff}"),
                      flush=True)
    print("ALL BIT-EQUAL" if equal else "OUTPUTS DIFFER")
    sys.exit(0 if equal else 1)

import torch  # noqa: E402
from ds2amd import _lib, ops  # noqa: E402

T, N, H, D = 501, 32, 800, 2
dev = torch.device("cuda")
g = torch.Generator(device="cpu").manual_seed(0)
xproj = (torch.randn(T, N, D, 3 * H, generator=g) * 0.5).to(dev)
w = [(torch.rand(3 * H, H, generator=g) * 0.06 - 0.03).to(dev) for _ in range(2)]
b = [(torch.rand(3 * H, generator=g) * 0.06 - 0.03).to(dev) for _ in range(2)]
lens = torch.full((N,), T, dtype=torch.int32, device=dev)
h_all = torch.empty(T, N, D, H, device=dev)
gates = torch.empty(T, N, D, 4 * H, device=dev)
dy = torch.randn(T, N, H, generator=g).to(dev)
dgx = torch.empty(T, N, D, 3 * H, device=dev)
dgh = torch.empty(T, N, D, 3 * H, device=dev)
wsf = torch.zeros(_lib.size("ds2_gru_fwd_workspace_size", N, H, D), dtype=torch.uint8, device=dev)
wsb = torch.zeros(_lib.size("ds2_gru_bwd_workspace_size", N, H, D), dtype=torch.uint8, device=dev)


def fwd():
    _lib.call("ds2_gru_fwd", T, N, H, D, xproj.data_ptr(), w[0].data_ptr(), w[1].data_ptr(),
              b[0].data_ptr(), b[1].data_ptr(), lens.data_ptr(), h_all.data_ptr(),
              gates.data_ptr(), None, wsf.data_ptr(), wsf.numel(), ops._stream())


def bwd():
    _lib.call("ds2_gru_bwd", T, N, H, D, dy.data_ptr(), 1, w[0].data_ptr(), w[1].data_ptr(),
              h_all.data_ptr(), gates.data_ptr(), lens.data_ptr(), dgx.data_ptr(),
              dgh.data_ptr(), None, wsb.data_ptr(), wsb.numel(), ops._stream())


def xl_modes():
    """The XCD-local kernels' per-group mode words (1 LOCAL, 2 GLOBAL, 3 mixed) of the last
    forward and backward launches, read from the workspaces' counter area."""
    if os.environ.get("DS2_GRU_XL", "1")[:1] == "0":
        return ""
    al = lambda x: (x + 255) & ~255
    UB, BT = (H + 15) // 16, (N + 15) // 16
    cf = al(D * UB * ((H + 3) // 4) * 3 * 64 * 4)
    cb = al(D * UB * ((3 * H + 3) // 4) * 64 * 4) + al(2 * N * D * H * 4)
    out = []
    for ws, c in ((wsf, cf), (wsb, cb)):
        words = ws[c:c + 4 * (D * BT + 1 + 520)].view(torch.int32).cpu()
        out.append(words[D * BT + 1 + 512: D * BT + 1 + 520].tolist())
    return f"  modes fwd {out[0]} bwd {out[1]}"


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def lib_child():
    import hashlib
    import json
    sha = lambda x: hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
    for (t, n, h, d) in LIB_SHAPES:
        gg = torch.Generator(device="cpu").manual_seed(1)
        xp = (torch.randn(t, n, d, 3 * h, generator=gg) * 0.5).to(dev)
        ww = [(torch.rand(3 * h, h, generator=gg) * 0.06 - 0.03).to(dev) for _ in range(2)]
        bb = [(torch.rand(3 * h, generator=gg) * 0.06 - 0.03).to(dev) for _ in range(2)]
        ln = torch.tensor([max(1, t - 3 * i) for i in range(n)], dtype=torch.int32, device=dev)
        dyy = torch.randn(t, n, h, generator=gg).to(dev)
        o = {k: torch.zeros(t, n, d, c * h, device=dev) for k, c in
             (("h_all", 1), ("gates", 4), ("dgx", 3), ("dgh", 3))}
        db = [torch.zeros(3 * h, device=dev) for _ in range(4)]
        col = torch.zeros(2 * d * 3 * h, dtype=torch.int32, device=dev)
        row = torch.zeros(t * n, dtype=torch.int32, device=dev)
        wf = torch.zeros(_lib.size("ds2_gru_fwd_workspace_size", n, h, d), dtype=torch.uint8, device=dev)
        wb = torch.zeros(_lib.size("ds2_gru_row_amax_workspace_size", t, n, h, d), dtype=torch.uint8, device=dev)

        def f():
            _lib.call("ds2_gru_fwd", t, n, h, d, xp.data_ptr(), ww[0].data_ptr(), ww[1].data_ptr(),
                      bb[0].data_ptr(), bb[1].data_ptr(), ln.data_ptr(), o["h_all"].data_ptr(),
                      o["gates"].data_ptr(), None, wf.data_ptr(), wf.numel(), ops._stream())

        def bk():
            _lib.call("ds2_gru_bwd_bias_amax", t, n, h, d, dyy.data_ptr(), 1, ww[0].data_ptr(),
                      ww[1].data_ptr(), o["h_all"].data_ptr(), o["gates"].data_ptr(), ln.data_ptr(),
                      o["dgx"].data_ptr(), o["dgh"].data_ptr(), db[0].data_ptr(), db[1].data_ptr(),
                      db[2].data_ptr(), db[3].data_ptr(), col.data_ptr(), None, wb.data_ptr(),
                      wb.numel(), ops._stream())

        tf = timed(f)
        tb = timed(bk)
        _lib.call("ds2_gru_row_amax", t, n, h, d, wb.data_ptr(), wb.numel(), row.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        hs = {k: sha(v) for k, v in o.items()}
        hs.update(col_amax=sha(col), row_amax=sha(row), dbias=sha(torch.cat(db)))
        print(json.dumps({"shape": f"{t}x{n}x{h}x{d}", "fwd_us": tf * 1e3, "bwd_us": tb * 1e3, "sha": hs}),
              flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "libchild":
    lib_child()
    sys.exit(0)

variants = {"x6": {"DS2_GRU_X6": "1", "DS2_RNN_TUNE": ""},
            "f32": {"DS2_GRU_X6": "0", "DS2_RNN_TUNE": ""}}
if len(sys.argv) > 1 and sys.argv[1] == "xcd":
    # the same-XCD groups vs the interleaved layout (DS2_GRU_XCD, read at every call)
    variants = {f"xcd{v}": {"DS2_GRU_X6": "1", "DS2_GRU_XCD": v} for v in ("1", "0")}
if len(sys.argv) > 1 and sys.argv[1] == "ftune":
    # the sentinel forward's first-poll delay / re-poll sleep (s_sleep units)
    variants = {f"fwd-tune-{t}": {"DS2_GRU_X6": "1", "DS2_RNN_TUNE": t}
                for t in ("1,10,14", "1,0,14", "1,4,14", "1,7,14", "1,14,14", "0,7,14", "2,7,14")}
if len(sys.argv) > 1 and sys.argv[1] == "flagpoll":
    # s_sleep(1) units between the flag hand-off's polls (the pre-split backward's wait)
    variants = {f"bwd-poll-{t}": {"DS2_GRU_X6": "1", "DS2_RNN_TUNE": t}
                for t in ("1,10,14,1", "1,10,14,0", "1,10,14,2", "1,10,14,4")}
if len(sys.argv) > 1 and sys.argv[1] == "flagpipe":
    # the flag hand-off with a second poll in flight, issued G s_sleep(1) units after the first
    # (0: one poll at a time)
    variants = {f"bwd-pipe-{g}": {"DS2_RNN_TUNE": f"1,10,14,1,{g}"} for g in ("0", "4", "8", "14", "20")}
if len(sys.argv) > 1 and sys.argv[1] == "flagdelay":
    # s_sleep(1) units before the backward's first flag poll of a step ([5]) and between polls ([3])
    variants = {f"bwd-flagdelay-{t}": {"DS2_RNN_TUNE": f"1,10,14,{t}"}
                for t in ("1,0,0", "1,0,8", "1,0,16", "1,0,24", "2,0,16", "4,0,16")}
if len(sys.argv) > 1 and sys.argv[1] == "xl":
    # the XCD-local kernels (gru_xl.hip) LOCAL (plain stores, default), forced GLOBAL (sc1), and
    # the 16-unit fp16x3 kernels they replace
    variants = {"xl-local": {"DS2_GRU_XL": "1", "DS2_RNN_TUNE": ""},
                "xl-global": {"DS2_GRU_XL": "2", "DS2_RNN_TUNE": ""},
                "16unit": {"DS2_GRU_XL": "0", "DS2_RNN_TUNE": ""}}
if len(sys.argv) > 1 and sys.argv[1] == "xlrepoll":
    # the XCD-local forward: tiles re-loaded per stale pass (DS2_RNN_TUNE [6]) x first-poll delay
    variants = {f"xl-rp-{t}": {"DS2_GRU_XL": "1", "DS2_RNN_TUNE": t}
                for t in ("1,7,14,1,0,0,8,7", "1,7,14,1,0,0,1,0", "1,7,14,1,0,0,2,0",
                          "1,7,14,1,0,0,1,3", "0,7,14,1,0,0,1,0", "1,7,14,1,0,0,8,0")}
if len(sys.argv) > 1 and sys.argv[1] == "xlonly":
    variants = {"xl-local": {"DS2_GRU_XL": "1", "DS2_RNN_TUNE": ""}}
if len(sys.argv) > 1 and sys.argv[1] == "xltune":
    # the XCD-local forward's first-poll delay / re-poll sleep (s_sleep units)
    variants = {f"xl-tune-{t}": {"DS2_GRU_XL": "1", "DS2_RNN_TUNE": t}
                for t in ("1,7,14", "1,0,14", "1,3,14", "0,0,14", "0,3,14", "2,3,14")}
rounds = int(os.environ.get("AB_ROUNDS", "3"))
variants = {f"{k}#{r}": v for r in range(rounds) for k, v in variants.items()}
ref = None
for name, env in variants.items():
    os.environ.update(env)
    tf = timed(fwd)
    out_h = h_all.clone()
    tb = timed(bwd)
    out_g = dgx.clone()
    if ref is None:
        ref = (out_h, out_g)
    dh = (out_h - ref[0]).abs().max().item()
    dg = (out_g - ref[1]).abs().max().item() / max(ref[1].abs().max().item(), 1e-30)
    print(f"{name:12s} fwd {tf * 1e3:8.1f} us ({tf * 1e3 / T:5.2f}/step)  bwd {tb * 1e3:8.1f} us "
          f"({tb * 1e3 / T:5.2f}/step)  max|dh| {dh:.2e} rel|ddgx| {dg:.2e}{xl_modes()}", flush=True)
