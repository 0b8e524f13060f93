"""Helpers of the streaming front-end tests (test_stream_frontend_cpu.py,
test_gpu_stream_frontend.py): csrc/stft_stream.hip's block constant restated, the geometries,
brute-force framing counts from np.pad(reflect), the partitions, and the causal 'max_frame'
definition restated in float64 and in float32 (their distance is the reference's own error,
which bounds the device as frontend_common's bound does: 4 e_ref + one float32 ulp of the
largest |value|).  The float64 restatement takes a `wrong=` switch: one deliberate mistake, for
the CPU file's sensitivity test."""
import collections
import functools

import numpy as np

from oracle import ds2_oracle as orc

import frontend_common as fc

SSF = 2                 # frames per stft_stream_kernel block (csrc/stft_stream.hip)
GAIN = 1048576.0        # 'max_frame': log1p(|X| 2^20)
# (n_fft, hop): the geometries the definition was checked on, and the ones the GPU tests run
GEOMETRIES = ((320, 160), (400, 160), (320, 80), (321, 160), (322, 7))
GPU_GEOMETRIES = GEOMETRIES[:3]
CONFS = {(320, 160): dict(sample_rate=16000, window_size=0.02, window_stride=0.01),
         (400, 160): dict(sample_rate=16000, window_size=0.025, window_stride=0.01),
         (320, 80): dict(sample_rate=16000, window_size=0.02, window_stride=0.005)}
LENGTHS = (1, 2, 160, 161, 319, 320, 321, 1280, 1281, 6400)
KINDS = ("ramp", "imp0", "impN", "silence")


# ------------------------------------------------------------------------------------------
# counts

def padded_index(n, n_fft, hop):
    """[T, n_fft]: the sample every tap of every frame of an n-sample utterance reads, from
    np.pad(reflect) and librosa's framing."""
    pad = n_fft // 2
    idx = np.pad(np.arange(n), pad, mode="reflect")
    t_n = fc.frames_of(n, n_fft, hop)
    return idx[np.arange(n_fft)[None, :] + hop * np.arange(t_n)[:, None]]


def final_frames_brute(a, n_fft, hop, longer):
    """Frames of an a-sample prefix that read the very samples the same frames of a longer
    utterance read (longer: its padded_index): those are final, the next one is not."""
    mine = padded_index(a, n_fft, hop)
    t = 0
    while t < len(mine) and np.array_equal(mine[t], longer[t]):
        t += 1
    return t


def final_frames_rule(a, n_fft, hop):
    """The issue's rule, frame by frame."""
    pad = n_fft // 2
    t = 0
    while max(t * hop - pad + n_fft - 1, pad - t * hop) <= a - 1:
        t += 1
    return t


def samples_for_frames(c, n_fft, hop):
    """The fewest samples at which c >= 1 frames are final (utterance open)."""
    pad = n_fft // 2
    return max(pad + 1, n_fft - pad) if c == 1 else n_fft - pad + (c - 1) * hop


# ------------------------------------------------------------------------------------------
# partitions of n samples: name -> chunk sizes (their sum is n; zeros are real empty feeds)

def _cut(sizes, n):
    out, left = [], n
    for s in sizes:
        s = min(s, left)
        out.append(s)
        left -= s
    if left:
        out.append(left)
    return out


def _by_frames(counts, n, n_fft, hop):
    """chunks after which 1 (frame 0), then counts[0], counts[1], ... more frames are final"""
    ends, c = [], 1
    ends.append(samples_for_frames(1, n_fft, hop))
    for k in counts:
        c += k
        ends.append(samples_for_frames(c, n_fft, hop))
    if ends[-1] > n:
        return None
    return _cut(list(np.diff([0] + ends)), n)


def partitions(n, n_fft, hop):
    p = {"all": [n], "mixed": _cut([159, 1, 1, 0, 160, 161], n)}
    if n <= 321:
        p["single"] = [1] * n
    # feeds that complete 7, 8, 9 frames, and SSF - 1, SSF, SSF + 1
    for name, counts in (("f789", (7, 8, 9)), ("fssf", (SSF - 1, SSF, SSF + 1, 2 * SSF + 1))):
        q = _by_frames(counts, n, n_fft, hop)
        if q is not None:
            p[name] = q
    # feeds that complete no frame: up to one sample before frame 0, and between frames
    gap = samples_for_frames(2, n_fft, hop) - samples_for_frames(1, n_fft, hop)
    p["zero"] = _cut([samples_for_frames(1, n_fft, hop) - 1, 1, gap - 1, 1, 0, hop - 1], n)
    return p


# ------------------------------------------------------------------------------------------
# the causal 'max_frame' definition

def _mags64(y, n_fft, hop):
    y = np.asarray(y, np.float32).astype(np.float64)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    t_n = fc.frames_of(len(y), n_fft, hop)
    idx = np.arange(n_fft)[None, :] + hop * np.arange(t_n)[:, None]
    return np.abs(np.fft.rfft(yp[idx] * orc.hamming(n_fft)[None, :], axis=1)).T[:fc.ROWS]


def causal_ref64(y, n_fft, hop, prior=(0.0, 0.0), wrong=None, calls=None):
    """val - off_t in float64 -> ([161, T], off [T], val [161, T]): val = log1p(|X| 2^20),
    m_t = mean over the 161 rows, S_t = S_{t-1} + m_t, off_t = (w o0 + S_t) / (w + t + 1).
    wrong: 'per_call' (one offset per feed, its last frame's; calls = the frames per feed),
    'one_indexed' (t counted from 1 in the denominator)."""
    o0, w = prior
    val = np.log1p(_mags64(y, n_fft, hop) * GAIN)
    s = np.cumsum(val.mean(axis=0))
    t = np.arange(val.shape[1]) + (2 if wrong == "one_indexed" else 1)
    off = (w * o0 + s) / (w + t)
    if wrong == "per_call":
        ends = np.cumsum(calls)
        off = np.concatenate([np.full(k, off[e - 1]) for k, e in zip(calls, ends) if k])
    return val - off[None, :], off, val


def causal_ref32(y, n_fft, hop, prior=(0.0, 0.0)):
    """The same chain with float32 where the device has float32: complex64 spectrum, float32
    magnitudes, log and frame means; the sum and the offset in float64, cast, subtracted in
    float32."""
    o0, w = prior
    mag = fc.stft_mag32(y, n_fft, hop)[:fc.ROWS]
    val = np.log1p(mag * np.float32(GAIN)).astype(np.float32)
    m = val.mean(axis=0, dtype=np.float32)
    s = np.cumsum(m.astype(np.float64))
    off = ((w * o0 + s) / (w + np.arange(val.shape[1]) + 1)).astype(np.float32)
    return (val - off[None, :]).astype(np.float64), val.astype(np.float64)


CausalRef = collections.namedtuple("CausalRef", "ref off val e_ref bound val_bound")


@functools.lru_cache(maxsize=None)
def causal_refs(kind, n, seed, n_fft, hop, prior=(0.0, 0.0)):
    """The float64 reference of one signal, the float32 restatement's distance from it and the
    device's bound (for the output, and for val alone)."""
    y = fc.signal(kind, n, seed, hop)
    ref, off, val = causal_ref64(y, n_fft, hop, prior)
    r32, v32 = causal_ref32(y, n_fft, hop, prior)
    e_ref = float(np.abs(r32 - ref).max())
    e_val = float(np.abs(v32 - val).max())
    ulp = lambda a: float(np.spacing(np.float32(np.abs(a).max())))
    return CausalRef(ref, off, val, e_ref, 4 * e_ref + ulp(ref), 4 * e_val + ulp(val))
