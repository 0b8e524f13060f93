"""Helpers of the audio front-end contract tests (test_gpu_frontend_contract.py,
test_frontend_contract_cpu.py): the spectrogram kernels of csrc/stft.hip, the librosa effects of
csrc/effects.hip and the waveform replay of csrc/wave.hip.  The case tables with the kernels'
block constants restated, the signals, plain float64 references (each STFT reference takes a
`wrong=` switch: one deliberate mistake, for the CPU file's sensitivity test), the bounds, and
runners that call the C entry points on operands inside poisoned allocations
(conv_common.Poisoned, head_common.PoisonedI32) with workspaces of exactly the query's bytes."""
import collections
import functools

import numpy as np
import torch

from ds2amd import _lib
from ds2amd import audio_aug as aa
from ds2amd import ops
from ds2amd.data_loader import gaussian_taps
from oracle import ds2_oracle as orc
from oracle import librosa_effects as le

from conv_common import Poisoned, Workspace
from head_common import (INVALID_VALUE, OK, UNSUPPORTED_SHAPE, WORKSPACE_TOO_SMALL,  # noqa: F401
                         PoisonedI32)

# csrc/stft.hip
SF = 8                 # frames per stft_kernel block
REMAP_COLS = 4         # columns (one wave each) per remap_kernel block
SUB_BLOCK = 256        # subtract_offset_kernel: threads per block ...
SUB_CAP = 512          # ... and the cap on its grid; above it the grid-stride loop takes a second trip
ROWS = 161
MAX_BINS = 256         # thread = bin: n_fft / 2 + 1 <= 256
MAX_NFFT = 1024
NORMS = ("none", "max_frame", "mean", "norm", "frame")      # ds2_stft_logmag modes 0..4
SIGMA = {1: 20, 4: 50}
NO_MASK = (0, 0, 0, 0, 0, 0, 0, 0, ROWS)
# csrc/effects.hip
FX_N, FX_HOP = 2048, 512
WING = 64              # zero crossings of one wing of resampy's kaiser_best filter
TREG_BLOCK = 64        # fx_treg_kernel: rows per block
# csrc/wave.hip
WAV_T = 1024
ERR_CAP, ERR_RECORD, ERR_LENGTH = 1, 2, 4        # the consistency word (ds2hip.h)


def frames_of(n, n_fft, hop):
    """librosa's count (center=True), as np.pad and the framing give it."""
    return 1 + (n + 2 * (n_fft // 2) - n_fft) // hop


def sub_blocks(max_frames):
    return -(-ROWS * max_frames // SUB_BLOCK)


# ------------------------------------------------------------------------------------------
# signals

KINDS = ("ramp", "imp0", "impN", "tone", "silence")


def signal(kind, n, seed, hop=160):
    """ramp: noise under an amplitude ramp 0.01 .. 1 with a burst over the first two frames, so
    the frame means differ most where the smoothing filter reflects; imp0 / impN: one sample of
    1.0 at either end, which a pad that repeated the edge would show twice; tone: the cosine of
    test_librosa_effects; silence: digital zero."""
    rng = np.random.default_rng(seed)
    if kind == "ramp":
        y = rng.standard_normal(n) * np.linspace(0.01, 1.0, n)
        k = min(n, 2 * hop)
        y[:k] += 3.0 * rng.standard_normal(k)
    elif kind in ("imp0", "impN"):
        # over a noise floor of 1e-3: a lone impulse has the same magnitude in every bin, so
        # 'norm' would divide by a standard deviation of rounding noise and the mean-subtracting
        # modes would leave rounding noise alone -- no reference is well-conditioned there
        y = 1e-3 * rng.standard_normal(n)
        y[0 if kind == "imp0" else n - 1] = 1.0
    elif kind == "tone":
        y = 0.5 * np.cos(2 * np.pi * 440.0 * np.arange(n) / 16000)
    elif kind == "silence":
        y = np.zeros(n)
    else:
        raise KeyError(kind)
    return y.astype(np.float32)


# ------------------------------------------------------------------------------------------
# STFT: the table.  One entry = one call = one ragged batch; every entry runs all five modes.

StftCase = collections.namedtuple("StftCase", "n_fft hop rows extra_frames extra_samples masks")


def _rows(lens, kinds=None, seed=0):
    kinds = kinds or KINDS
    return tuple((n, kinds[i % len(kinds)], seed + i) for i, n in enumerate(lens))


def _case(n_fft, hop, rows, extra_frames=0, extra_samples=0, masks=None):
    return StftCase(n_fft, hop, rows, extra_frames, extra_samples, masks)


def _mask_rows(t):
    """Hand-written mask rows for an utterance of t frames (ds2hip.h: {f_lo0, f_hi0, f_lo1, f_hi1,
    t_lo0, t_hi0, t_lo1, t_hi1, f_cut})."""
    return ((5, 5, 0, 0, 3, 3, 0, 0, ROWS),                      # empty bands
            (0, 1, 160, 161, 0, 0, 0, 0, ROWS),                  # the first and the last row
            (0, 0, 0, 0, 0, 1, t - 1, t, ROWS),                  # the first and the last frame
            (0, 0, 0, 0, t - 1, t + 1, 0, 0, ROWS),              # one past T
            (10, 40, 30, 60, 2, 5, 4, 7, ROWS),                  # overlapping
            (0, 0, 0, 0, 0, 0, 0, 0, 0),                         # f_cut 0: everything masked
            (3, 9, 0, 0, 1, 2, 0, 0, 81),                        # the 8 kHz cut
            (0, 0, 0, 0, 0, 0, 0, 0, 161))


MASK_T = 9
STFT_CASES = {
    # fused, F = 161.  pad 160: n = 1, 2 fold it many times, 160 twice, 161 exactly once
    "f320": _case(320, 160, _rows((1, 2, 159, 160, 161, 1119, 1120, 1280, 2560)), 3, 5),
    # T = 816: the subtract grid is capped and its loop takes a second trip
    "f320_hop16": _case(320, 16, _rows((16 * 815, 37), ("ramp", "tone"), 20)),
    # odd n_fft: hop divides 220 and 2200, where 1 + n / hop counts one frame too many
    "f441": _case(441, 220, _rows((1, 219, 220, 2199, 2200, 2201),
                                  ("ramp", "imp0", "impN", "silence", "tone"), 40)),
    "f510": _case(510, 255, _rows((300,), ("ramp",), 60)),
    # remap path (F < 161): T = 1, 3, 4, 5 around the 4-column block; 2 hop and 4 hop are multiples
    "r160": _case(160, 80, _rows((79, 160, 247, 320), None, 80), 3, 9),
    "r319": _case(319, 159, _rows((159, 477, 636, 700), None, 100)),
    "r220": _case(220, 110, _rows((109, 220, 337, 440), ("silence", "impN", "ramp", "tone"), 120)),
    "r80": _case(80, 40, _rows((39, 80, 127, 160), None, 140)),
    "r2": _case(2, 1, _rows((5,), ("ramp",), 160)),
    # the hand-written mask rows, one utterance of MASK_T frames each, on both paths
    "f320_masks": _case(320, 160, _rows((1280,) * 8, ("ramp",), 180), masks=_mask_rows(MASK_T)),
    "r160_masks": _case(160, 80, _rows((640,) * 8, ("ramp",), 200), masks=_mask_rows(MASK_T)),
}


def case_frames(case):
    c = STFT_CASES[case]
    return [frames_of(n, c.n_fft, c.hop) for n, _, _ in c.rows]


def case_signals(case):
    c = STFT_CASES[case]
    return [signal(kind, n, seed, c.hop) for n, kind, seed in c.rows]


# ------------------------------------------------------------------------------------------
# STFT: references

def _masked(s, row, inclusive=False):
    r = np.arange(s.shape[0])[:, None]
    t = np.arange(s.shape[1])[None, :]
    e = 1 if inclusive else 0          # the mistake: a band [lo, hi] where it is not empty
    m = np.broadcast_to(r >= row[8], s.shape).copy()
    for i in (0, 2):
        if row[i] < row[i + 1]:
            m |= (r >= row[i]) & (r < row[i + 1] + e)
        if row[4 + i] < row[5 + i]:
            m |= (t >= row[4 + i]) & (t < row[5 + i] + e)
    return np.where(m, 0.0, s)


def stft_ref64(y, n_fft, hop, mode, mask=NO_MASK, wrong=None):
    """normalize_audio(rows161(|librosa.stft(y)|)) in float64 throughout -> [161, T].  wrong: one
    deliberate mistake (test_frontend_contract_cpu's sensitivity test)."""
    from scipy.ndimage import gaussian_filter1d
    y = np.asarray(y, np.float32).astype(np.float64)
    pad = n_fft // 2
    t_n = 1 + len(y) // hop if wrong == "frames" else frames_of(len(y), n_fft, hop)
    # the extra hop on the right feeds the one frame too many of wrong == "frames" only
    yp = np.pad(y, (pad, pad + hop), mode="symmetric" if wrong == "edge_pad" else "reflect")
    idx = np.arange(n_fft)[None, :] + hop * np.arange(t_n)[:, None]
    mag = np.abs(np.fft.rfft(yp[idx] * orc.hamming(n_fft)[None, :], axis=1))     # [T, F]
    f = mag.shape[1]
    if f < ROWS:
        # ndarray.resize on the Fortran-ordered [F, T] matrix: its frame-major memory, cut or
        # zero-filled to 161 T values, read column-major; then rows 81.. mirror rows 80..1
        flat = np.zeros(ROWS * t_n)
        k = min(flat.size, mag.size)
        flat[:k] = mag.reshape(-1)[:k]
        s = flat.reshape(ROWS, t_n) if wrong == "row_major" else flat.reshape(t_n, ROWS).T.copy()
        s[81:] = s[79::-1] if wrong == "mirror" else s[80:0:-1]
    else:
        s = mag.T[:ROWS].copy()
    s = _masked(s, mask, inclusive=wrong == "mask_hi")
    if mode == 1:
        s = np.log1p(s) * 1048576.0 if wrong == "gain" else np.log1p(s * 1048576.0)
    else:
        s = np.log1p(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode in (1, 4):
            sm = gaussian_filter1d(s.mean(axis=0), SIGMA[mode],
                                   mode="mirror" if wrong == "np_reflect" else "reflect")
            s = s - sm.mean()
        elif mode == 2:
            s = s - s.mean()
        elif mode == 3:
            s = s - s.mean()
            s = s / s.std(axis=0, ddof=0 if wrong == "biased_std" else 1).mean()
    return s


def stft_mag32(y, n_fft, hop):
    """orc.stft_magnitude with the geometry given, not derived from a sample rate."""
    y = np.asarray(y, dtype=np.float32)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    n_frames = 1 + (len(yp) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    frames = yp[idx].astype(np.float64) * orc.hamming(n_fft)[None, :]
    return np.abs(np.fft.rfft(frames, axis=1).astype(np.complex64).T)


def stft_ref32(y, n_fft, hop, mode, mask=NO_MASK):
    """The oracle's float32 chain (orc.spectrogram's: rows161, the reference's mask slices,
    normalize_audio) -> float64 copy of its float32 result."""
    from ds2amd.spect_aug import apply_masks_np
    mag = np.array(orc.rows161(stft_mag32(y, n_fft, hop)))
    if tuple(mask) != NO_MASK:
        mag = apply_masks_np(mag, mask)
    with np.errstate(invalid="ignore", divide="ignore"):
        return orc.normalize_audio(mag, NORMS[mode]).numpy().astype(np.float64)


def same_nans(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))


def max_diff(a, b):
    """max |a - b| over the elements finite in both, the shorter one zero-padded in time (a
    reference with a wrong frame count still compares); inf where only one is NaN."""
    t = max(a.shape[1], b.shape[1])
    a = np.pad(a, ((0, 0), (0, t - a.shape[1])))
    b = np.pad(b, ((0, 0), (0, t - b.shape[1])))
    if not same_nans(a, b):
        return float("inf")
    d = np.abs(a - b)[~np.isnan(a)]
    return float(d.max()) if d.size else 0.0


StftRef = collections.namedtuple("StftRef", "ref r32 e_ref bound")


@functools.lru_cache(maxsize=None)
def stft_refs(case, mode):
    """Per row of the case: the float64 reference, the oracle-style float32 one, their distance
    e_ref and the device's bound 4 e_ref + one float32 ulp of the reference's largest |value|."""
    c = STFT_CASES[case]
    out = []
    for i, y in enumerate(case_signals(case)):
        mask = c.masks[i] if c.masks else NO_MASK
        ref = stft_ref64(y, c.n_fft, c.hop, mode, mask)
        r32 = stft_ref32(y, c.n_fft, c.hop, mode, mask)
        e_ref = max_diff(r32, ref)
        fin = np.abs(ref[np.isfinite(ref)])
        top = np.float32(fin.max()) if fin.size else np.float32(0)
        out.append(StftRef(ref, r32, e_ref, 4 * e_ref + float(np.spacing(top))))
    return out


# ------------------------------------------------------------------------------------------
# STFT: the runner

def _i32(v, dev):
    return PoisonedI32(torch.tensor(v, dtype=torch.int32), dev)


def run_stft(case, mode, dev, rows=None, entry="ds2_stft_logmag_masked"):
    """One call of the case's batch (or of the given rows of it alone) -> [B, 161, max_frames]
    float32 on the host.  pcm holds NaN past every row's samples, out NaN everywhere before the
    launch, the workspace is the query's bytes exactly; canaries are checked here."""
    c = STFT_CASES[case]
    pick = list(range(len(c.rows))) if rows is None else list(rows)
    sigs = [case_signals(case)[i] for i in pick]
    lens = [len(y) for y in sigs]
    max_samples = max(lens) + c.extra_samples
    max_frames = max(frames_of(n, c.n_fft, c.hop) for n in lens) + c.extra_frames
    host = torch.full((len(sigs), max_samples), float("nan"))
    for i, y in enumerate(sigs):
        host[i, :len(y)] = torch.from_numpy(y)
    pcm = Poisoned(host, dev)
    ns = _i32(lens, dev)
    win = torch.from_numpy(orc.hamming(c.n_fft)).to(dev)
    taps = None
    if mode in SIGMA:
        taps = torch.from_numpy(gaussian_taps(SIGMA[mode]).astype(np.float32)).to(dev)
    radius = 0 if taps is None else (taps.numel() - 1) // 2
    masks = None if c.masks is None else _i32([c.masks[i] for i in pick], dev)
    out = Poisoned((len(sigs), ROWS, max_frames), dev)
    ws = Workspace(_lib.size("ds2_stft_workspace_size", len(sigs), max_frames, c.n_fft), dev)
    args = [pcm.ptr, ns.ptr, len(sigs), max_samples, c.n_fft, c.hop, win.data_ptr(), mode,
            None if taps is None else taps.data_ptr(), radius]
    if entry == "ds2_stft_logmag_masked":
        args.append(None if masks is None else masks.ptr)
    else:
        assert masks is None
    _lib.call(entry, *args, out.ptr, max_frames, ws.ptr, ws.nbytes, None)
    torch.cuda.synchronize()
    assert out.intact(), f"{case}: a write outside out"
    assert ws.intact(), f"{case}: a write outside the workspace"
    return out.read().numpy()


# ------------------------------------------------------------------------------------------
# time stretch

STRETCH_ROWS = ((1, 1.0, "imp0"), (2, 0.85, "ramp"), (511, 1.15, "tone"), (512, 1.0, "ramp"),
                (513, 0.93, "impN"), (1023, 1.07, "ramp"), (1024, 0.5, "tone"), (1025, 2.0, "ramp"),
                (3000, 4.0, "tone"), (5000, 3.0, "ramp"),
                (3072, 0.2, "ramp"),       # the ISTFT's length limit: used 34 < 35 frames
                (1024, 0.1, "tone"),       # 30 steps, used 24; the last one's second column is padding
                (4096, 0.072, "ramp"))     # 9 / 0.072 rounds above 125: a 126th step, at 125 * 0.072
#                                            = 9.0, has both columns in the padding (used 116)
STRETCH_X_EXTRA = 7


def stretch_signals():
    return [signal(kind, n, 300 + i, FX_HOP) for i, (n, _, kind) in enumerate(STRETCH_ROWS)]


def rel_diff(got, exp):
    """test_librosa_effects._cmp: max |got - exp| over the peak of exp."""
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def stretch_refs():
    """Per row: (restatement, float64 chain, noise = their relative distance)."""
    out = []
    for y, (_, rate, _) in zip(stretch_signals(), STRETCH_ROWS):
        e, f = le.time_stretch(y, rate), le.time_stretch_f64(y, rate)
        out.append((e, f, rel_diff(e, f)))
    return out


def run_stretch(dev, rows=None):
    """ds2_time_stretch on the table's ragged batch (or the given rows alone), x_stride above
    the longest row -> ([N, out_stride] host array, out_lens)."""
    pick = list(range(len(STRETCH_ROWS))) if rows is None else list(rows)
    sigs = [stretch_signals()[i] for i in pick]
    lens = [len(y) for y in sigs]
    rates = [STRETCH_ROWS[i][1] for i in pick]
    plans = [ops.stretch_plan(n, r) for n, r in zip(lens, rates)]
    x_stride = max(lens) + STRETCH_X_EXTRA
    host = torch.full((len(sigs), x_stride), float("nan"))
    for i, y in enumerate(sigs):
        host[i, :len(y)] = torch.from_numpy(y)
    x = Poisoned(host, dev)
    out_stride = max(p[0] for p in plans) + 3
    max_in = max(1 + n // FX_HOP for n in lens)
    max_out = max(p[1] for p in plans)
    out = Poisoned((len(sigs), out_stride), dev)
    ws = Workspace(_lib.size("ds2_time_stretch_workspace_size", len(sigs), max_in, max_out), dev)
    rate_d = torch.tensor(rates, dtype=torch.float64).to(dev)
    win = torch.from_numpy(ops.hann_periodic(FX_N)).to(dev)
    ld, of, uf, ol = (_i32(v, dev) for v in (lens, [p[1] for p in plans], [p[2] for p in plans],
                                             [p[0] for p in plans]))
    _lib.call("ds2_time_stretch", x.ptr, x_stride, ld.ptr, len(sigs), rate_d.data_ptr(), of.ptr,
              uf.ptr, ol.ptr, win.data_ptr(), out.ptr, out_stride, max_in, max_out, ws.ptr,
              ws.nbytes, None)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    return out.read().numpy(), [p[0] for p in plans]


# ------------------------------------------------------------------------------------------
# resample

RESAMPLE_LENS = (1, 2, 63, 64, 65, 129, 777)
RESAMPLE_PAIRS = ((8000, 16000), (16000, 8000), (22050, 16000), (16000, 16000), (16000, 17959.5),
                  (44100, 16000))          # ratios 2, 0.5, 0.7256, 1, 1.1225, 0.3628
ResampleRow = collections.namedtuple("ResampleRow", "n pair valid out_len")


def _resample_rows(stride, lens, pairs):
    rows = []
    for i, (n, pair) in enumerate((n, p) for n in lens for p in pairs):
        valid = le.resample_length(n, *pair)
        # every third row asks for one sample fewer than resampy gives; the others for the
        # whole stride, which is below the resampled length of the long rows and above the rest
        out_len = min(stride, max(valid - 1, 0)) if i % 3 == 0 else stride
        rows.append(ResampleRow(n, pair, valid, out_len))
    return rows


RESAMPLE_BATCHES = {
    "s256": (256, _resample_rows(256, RESAMPLE_LENS, RESAMPLE_PAIRS)),
    "s257": (257, _resample_rows(257, RESAMPLE_LENS, RESAMPLE_PAIRS)),
    # fx_treg_kernel's second block
    "rows65": (8, _resample_rows(8, (2,) * 65, RESAMPLE_PAIRS[:1])[:65]),
}


def resample_signal(batch, i):
    n = RESAMPLE_BATCHES[batch][1][i].n
    return signal("ramp", n, 500 + i, 16)


@functools.lru_cache(maxsize=None)
def resample_refs(batch):
    return [le.resampy_resample(resample_signal(batch, i), *r.pair)
            for i, r in enumerate(RESAMPLE_BATCHES[batch][1])]


def run_resample(batch, dev):
    stride, rows = RESAMPLE_BATCHES[batch]
    x_stride = max(r.n for r in rows) + 5
    host = torch.full((len(rows), x_stride), float("nan"))
    for i, r in enumerate(rows):
        host[i, :r.n] = torch.from_numpy(resample_signal(batch, i))
    x = Poisoned(host, dev)
    out = Poisoned((len(rows), stride), dev)
    ws = Workspace(_lib.size("ds2_resample_workspace_size", len(rows), stride), dev)
    win, nb = ops.kaiser_best_filter()
    win = torch.from_numpy(np.ascontiguousarray(win)).to(dev)
    ratio = torch.tensor([float(r.pair[1]) / r.pair[0] for r in rows], dtype=torch.float64).to(dev)
    ld = _i32([r.n for r in rows], dev)
    nv = _i32([min(r.valid, r.out_len) for r in rows], dev)
    _lib.call("ds2_resample", x.ptr, x_stride, ld.ptr, len(rows), ratio.data_ptr(), nv.ptr,
              win.data_ptr(), win.numel(), nb, out.ptr, stride, ws.ptr, ws.nbytes, None)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    return out.read().numpy()


# ------------------------------------------------------------------------------------------
# wave aug.  A row = (samples, [records]); a record = (kind, a, b, alpha): SHIFT (shift, limit),
# DISTORT alpha, NOISE (noise row, -, alpha).

S, D, N = aa.SHIFT, aa.DISTORT, aa.NOISE


def _neg(n, seed):
    return -np.abs(signal("ramp", n, seed)) - np.float32(0.01)


def _last_max(n, seed):
    y = signal("ramp", n, seed)
    y[-1] = np.abs(y).max() + np.float32(1.0)
    return y


def wave_rows():
    full = [(S, 0, 3, 0.0), (D, 0, 0, 1.02), (N, 0, 0, 0.1), (S, 2, 2, 0.0)]
    return [
        (signal("ramp", 1, 700), full),
        (signal("ramp", 63, 701), [(S, 5, 5, 0.0), (D, 0, 0, 0.97), (N, 1, 0, 0.2), (S, 0, 0, 0.0)]),
        (signal("ramp", 1023, 702), [(D, 0, 0, 1.03), (D, 0, 0, 0.95)]),
        (signal("ramp", 1024, 703), [(N, 2, 0, 0.15)]),           # rows 3 and 4 share noise row 2
        (signal("ramp", 1025, 704), [(N, 2, 0, 0.05)]),
        (signal("ramp", 2049, 705), []),                          # END first: a plain copy
        (_neg(1025, 706), [(D, 0, 0, 1.04)]),                     # all negative: clip's min > max
        (_last_max(1024, 707), [(D, 0, 0, 0.5)]),                 # the maximum is the last sample
        (signal("tone", 2049, 708), [(S, 0, 0, 0.0), (D, 0, 0, 1.01), (N, 3, 0, 0.12), (S, 7, 7, 0.0)]),
    ]


WAVE_NOISE_ROWS = 4
WAVE_MAX_OPS = 4


def wave_noise():
    return np.random.default_rng(720).standard_normal((WAVE_NOISE_ROWS, 2100))


def wave_lengths(y, recs):
    """(final length, longest intermediate length)."""
    ln = cap = len(y)
    for kind, a, b, alpha in recs:
        if kind == S:
            ln += b
        cap = max(cap, ln)
    return ln, cap


def wave_ref(y, recs, noise):
    """tests/test_audio_aug.py::_replay on the row's records."""
    from test_audio_aug import _replay
    w = aa.Wave(y)
    ln = len(y)
    for kind, a, b, alpha in recs:
        if kind == S:
            ln += b
        w.records.append((kind, a, b, alpha, noise[a, :ln] if kind == N else None))
    return _replay(w)


def wave_ops(rows, max_ops=WAVE_MAX_OPS):
    op_i = np.zeros((len(rows), max_ops, 4), np.int32)
    op_f = np.zeros((len(rows), max_ops), np.float64)
    for r, (_, recs) in enumerate(rows):
        for j, (kind, a, b, alpha) in enumerate(recs):
            op_i[r, j] = (kind, a, b, 0)
            op_f[r, j] = alpha
    return op_i, op_f


def run_wave(rows, noise, dev, cap=None, out_lens=None, in_lens=None):
    """ds2_wave_aug on the rows -> (out [N, out_stride] on the host, still NaN where nothing was
    written; the consistency word).  in_stride and out_stride above every row; cap the longest
    intermediate length exactly unless given."""
    lens = [len(y) for y, _ in rows]
    finals = [wave_lengths(y, recs) for y, recs in rows]
    cap = max(c for _, c in finals) if cap is None else cap
    out_lens = [f for f, _ in finals] if out_lens is None else out_lens
    in_stride = max(lens) + 3
    out_stride = max(max(out_lens), 1) + 5
    host = torch.full((len(rows), in_stride), float("nan"))
    for i, (y, _) in enumerate(rows):
        host[i, :len(y)] = torch.from_numpy(y)
    x = Poisoned(host, dev)
    op_i, op_f = wave_ops(rows)
    oi = _i32(op_i.tolist(), dev)
    of = torch.from_numpy(op_f).to(dev)
    nz = None if noise is None else torch.from_numpy(noise).to(dev)
    out = Poisoned((len(rows), out_stride), dev)
    ws = Workspace(_lib.size("ds2_wave_aug_workspace_size", len(rows), cap), dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    il, ol = _i32(lens if in_lens is None else in_lens, dev), _i32(out_lens, dev)
    _lib.call("ds2_wave_aug", x.ptr, in_stride, il.ptr, len(rows), oi.ptr, of.data_ptr(),
              WAVE_MAX_OPS, None if nz is None else nz.data_ptr(),
              0 if nz is None else nz.stride(0), out.ptr, out_stride, ol.ptr, cap,
              err.data_ptr(), ws.ptr, ws.nbytes, None)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    return out.read().numpy(), int(err.item())
