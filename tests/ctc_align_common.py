"""CPU restatement of CTC forced alignment (ds2_ctc_align) and the seeded inputs that the CPU
and GPU tests share.

`viterbi` is the max-plus dynamic programme over the extended label sequence with the tie
rule of include/ds2hip.h: a predecessor replaces the best so far only if strictly greater,
tried in the order stay, s - 1, s - 2; the final state is S - 1 unless v(S - 2) > v(S - 1).
It runs in a chosen dtype, optionally rescaled as the kernel rescales (every `rescale`-th row
has the previous row's maximum subtracted, the subtracted amounts summed in float64); the
float64 unrescaled run is the reference.  Log-probabilities are torch's float64 log-softmax.

The kernel's constants decide the shapes of `_CASES`: 512 threads each owning states
tid + 512 k, log-probabilities staged 256 frames at a time, a row rescaled every 8th step,
back-pointers staged 128 frames at a time, label offsets summed 64 utterances per trip.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

COST_RTOL = 1e-6          # the project's bound for CTC costs (tests/test_gpu_ctc.py)
RESCALE = 8               # kScanRescale
BP_CHUNK = 128            # kAlignChunk


# ---------------------------------------------------------------------------- reference
def log_probs64(acts):
    """float64 log-softmax over the classes of acts [..., C] (numpy float64)."""
    return F.log_softmax(acts.detach().double(), dim=-1).numpy()


def need(labels):
    """Frames a label sequence needs at least: L + the number of adjacent equal labels."""
    lab = [int(v) for v in labels]
    return len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def viterbi(lp, labels, blank=0, dtype=np.float64, rescale=0):
    """Best alignment of `labels` to the T rows of lp [T, C] (float64 log-probabilities,
    rounded to `dtype` first).  Returns (states, score): states a list of T extended states,
    or None when the labels do not fit (score -inf); score a float64.  T = 0 with no labels is
    ([], 0.0)."""
    lab = [int(v) for v in labels]
    t_n, l_n = lp.shape[0], len(lab)
    s_n = 2 * l_n + 1
    if t_n == 0:
        return ([], 0.0) if l_n == 0 else (None, -np.inf)
    ext = np.full(s_n, blank, dtype=np.int64)
    ext[1::2] = lab
    skip = np.zeros(s_n, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    lp = lp.astype(dtype)
    ninf = dtype(-np.inf)
    v = np.full(s_n, ninf, dtype=dtype)
    v[:2] = lp[0, ext[:2]]
    bp = np.zeros((t_n, s_n), dtype=np.uint8)
    off = 0.0
    for t in range(1, t_n):
        msub = dtype(0)
        if rescale and t % rescale == 0:
            m = v.max()
            if m != ninf:
                msub = m
            off += float(msub)
        best = v.copy()
        d = np.zeros(s_n, dtype=np.uint8)
        one = np.full(s_n, ninf, dtype=dtype)
        one[1:] = v[:-1]
        m1 = one > best
        best[m1] = one[m1]
        d[m1] = 1
        two = np.full(s_n, ninf, dtype=dtype)
        two[2:] = v[:-2]
        m2 = skip & (two > best)
        best[m2] = two[m2]
        d[m2] = 2
        with np.errstate(invalid="ignore"):
            nv = best + (lp[t, ext] - msub)
        nv[best == ninf] = ninf
        v = nv.astype(dtype)
        bp[t] = d
    s = s_n - 1
    if s_n >= 2 and v[s_n - 2] > v[s_n - 1]:
        s = s_n - 2
    if v[s] == ninf:
        return None, -np.inf
    score = float(v[s]) + off
    states = [0] * t_n
    for t in range(t_n - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return states, score


def frame_labels(states, labels, blank=0):
    return [int(labels[s >> 1]) if s & 1 else blank for s in states]


def collapse(frames, blank=0):
    out, prev = [], None
    for f in frames:
        if f != prev and f != blank:
            out.append(f)
        prev = f
    return out


def path_score64(lp, states, labels, blank=0):
    """float64 log-probability of a state path."""
    return float(sum(lp[t, c] for t, c in enumerate(frame_labels(states, labels, blank))))


def spans_of(states, n_labels):
    """[first frame, one past the last] of every label's state 2 i + 1."""
    out = []
    for i in range(n_labels):
        fr = [t for t, s in enumerate(states) if s == 2 * i + 1]
        out.append([fr[0], fr[-1] + 1])
    return out


def validity_errors(states, labels, blank=0):
    """Why `states` is not a valid CTC alignment of `labels` ([] when it is)."""
    lab = [int(v) for v in labels]
    s_n = 2 * len(lab) + 1
    errs = []
    if not states:
        return errs if not lab else ["no frames"]
    if states[0] not in (0, 1) or states[0] >= s_n:
        errs.append(f"start state {states[0]}")
    if states[-1] not in (s_n - 1, s_n - 2) or states[-1] < 0:
        errs.append(f"end state {states[-1]} of {s_n}")
    for t in range(1, len(states)):
        a, b = states[t - 1], states[t]
        if b - a not in (0, 1, 2) or not 0 <= b < s_n:
            errs.append(f"step {a} -> {b} at frame {t}")
        elif b - a == 2 and not (b & 1 and lab[b >> 1] != lab[(b >> 1) - 1]):
            errs.append(f"skip {a} -> {b} at frame {t} not allowed")
    if not errs and collapse(frame_labels(states, lab, blank), blank) != lab:
        errs.append("frame labels do not collapse to the target")
    return errs


def brute_force(lp, labels, blank=0):
    """The best of all C^T frame labellings that collapse to `labels`: (frames, score), or
    (None, -inf) when there is none."""
    t_n, c = lp.shape
    lab = [int(v) for v in labels]
    best, best_fr = -np.inf, None
    for code in range(c ** t_n):
        fr = [(code // c ** t) % c for t in range(t_n)]
        if collapse(fr, blank) != lab:
            continue
        sc = float(sum(lp[t, f] for t, f in enumerate(fr)))
        if sc > best:
            best, best_fr = sc, fr
    return best_fr, best


# ---------------------------------------------------------------------------- inputs
def _draw(gen, length, c, blank):
    """`length` labels that avoid the blank: C - 1 values, those >= blank shifted up by one."""
    v = torch.randint(0, c - 1, (length,), generator=gen, dtype=torch.int32)
    return v + (v >= blank).int()


def _pack(acts, labels, act, blank):
    return SimpleNamespace(
        acts=acts, labels=torch.cat(labels).int() if labels else torch.zeros(0, dtype=torch.int32),
        per_sample=labels, blank=blank, act_lens=torch.tensor(act, dtype=torch.int32),
        label_lens=torch.tensor([int(v.numel()) for v in labels], dtype=torch.int32))


def _case(seed, t, c, act, lab, blank=0, scale=2.0, labels=None):
    gen = torch.Generator().manual_seed(seed)
    acts = torch.randn(t, len(act), c, generator=gen) * scale
    if labels is None:
        labels = [_draw(gen, n, c, blank) for n in lab]
    return _pack(acts, labels, act, blank)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _degenerate():
    """C = 6, t_max = 12: L = 0; T = 0 with L = 0; T = 0 with L = 2; labels that need 8 frames
    given 7 (infeasible) and exactly 8 (one path); act_len < t_max; act_len > t_max (clamped)."""
    rep = [2, 2, 3, 3, 3]
    labels = [_i32([]), _i32([]), _i32([1, 5]), _i32(rep), _i32(rep), _i32([4, 1, 1]),
              _i32([3, 2, 5])]
    assert need(rep) == 8
    return _case(70, 12, 6, [12, 0, 0, 7, 8, 7, 20], None, labels=labels)


def _planted(seed, t, l_n, c, blank=0):
    """Noise of 0.1 plus 12 on the classes of a drawn valid alignment: that alignment wins by
    a wide margin.  Returns the case and the planted states."""
    gen = torch.Generator().manual_seed(seed)
    lab = _draw(gen, l_n, c, blank)
    s_n = 2 * l_n + 1
    # frames per extended state: 1 per label, 1 per blank between equal labels, the rest
    # of the T frames thrown at random states
    dur = [0] * s_n
    for i in range(l_n):
        dur[2 * i + 1] = 1
        if i and int(lab[i]) == int(lab[i - 1]):
            dur[2 * i] = 1
    extra = t - sum(dur)
    assert extra >= 0
    for s in torch.randint(0, s_n, (extra,), generator=gen).tolist():
        dur[s] += 1
    states = [s for s in range(s_n) for _ in range(dur[s])]
    acts = torch.randn(t, 1, c, generator=gen) * 0.1
    for f, k in enumerate(frame_labels(states, lab.tolist(), blank)):
        acts[f, 0, k] += 12.0
    return _pack(acts, [lab], [t], blank), states


# name -> builder; the comment says which path of ctc_align_kernel the case executes
_CASES = {
    "degenerate": _degenerate,
    # S = 511 / 513 / 515 straddle thread 511 | 512; the first back-trace chunk starts at
    # s_hi > 256, so its staged window begins past the row's start
    "ownership": lambda: _case(71, 300, 29, [300, 300, 290], [255, 256, 257]),
    # S = 2049: all five k of the state loop, 11 back-trace chunks, a 2052-byte row
    "full_states": lambda: _case(72, 1400, 5, [1400], [1024]),
    # kScanRescale = 8: no subtraction (1, 7, 8), the first on the last row (9), 16, 17
    "rescale_edges": lambda: _case(73, 17, 29, [1, 7, 8, 9, 16, 17], [1, 3, 4, 4, 2, 3]),
    # a full log-probability stage and one frame more
    "stage_edges": lambda: _case(74, 257, 29, [255, 256, 257], [40, 40, 40]),
    # kAlignChunk = 128: a chunk short of one frame, full, and a one-frame second chunk
    "bp_chunk_edges": lambda: _case(75, 129, 29, [127, 128, 129], [20, 64, 30]),
    # the benchmark's length at three logit scales (peaked, moderate, nearly flat)
    "bench_len": lambda: _case(76, 501, 29, [501], [150]),
    "bench_len_s05": lambda: _case(77, 501, 29, [501], [150], scale=0.5),
    "bench_len_s005": lambda: _case(78, 501, 29, [501], [150], scale=0.05),
    # C = 64 (the staged frames fill lpc), the blank in the last lane
    "c64_blank63": lambda: _case(79, 300, 64, [300, 257], [256, 100], blank=63),
    # C = 2: one label, every neighbour a repeat, no skip transition anywhere
    "c2_repeats": lambda: _case(80, 40, 2, [40, 17, 9, 1], [10, 6, 0, 1], blank=0),
    "blank_mid": lambda: _case(81, 50, 10, [50, 20, 8], [7, 3, 0], blank=4),
    # the prep kernel's label-offset sum takes a second trip for utterance 64
    "many_utts": lambda: _case(82, 40, 29, [40 - i % 9 for i in range(65)],
                               [i % 7 for i in range(65)]),
    # all-zero logits: every alignment ties exactly, the tie rule alone picks the path
    "ties": lambda: _zeros(_case(83, 24, 6, [24, 20, 9, 24], None,
                                 labels=[_i32([1, 1, 2, 3, 3, 3, 4, 5, 1, 2]),
                                         _i32([2, 2, 4, 1, 5]), _i32([]), _i32([3] * 12)])),
    "planted": lambda: _planted(84, 140, 30, 29)[0],
}
CASE_NAMES = list(_CASES)


def _zeros(k):
    k.acts = torch.zeros_like(k.acts)
    return k


@functools.lru_cache(maxsize=None)
def ties_long():
    """All-zero logits over more frames than a back-trace chunk and 17 rescalings.  Kept out
    of _CASES: every step adds the same -log C, so the roundings of an unrescaled float32 sum
    do not average out and its score drifts to 1.6e-6 relative at T = 140, past the bound that
    the rescaled sum (the kernel's) keeps.  Returns the case and its float64 reference."""
    k = _zeros(_case(85, 140, 6, [140, 130], None,
                     labels=[_i32([1, 1, 2, 3, 3, 3, 4, 5, 1, 2] * 3), _i32([3] * 40)]))
    lp = log_probs64(k.acts)
    return k, lp, [viterbi(lp[:t, b], lab, k.blank) for b, t, lab in utterances(k)]


@functools.lru_cache(maxsize=None)
def make_case(name):
    return _CASES[name]()


def utterances(k):
    """(b, T, labels) of every utterance of a case, T clamped to the acts' frames."""
    t_max = k.acts.shape[0]
    return [(b, min(max(int(k.act_lens[b]), 0), t_max), [int(v) for v in k.per_sample[b]])
            for b in range(len(k.per_sample))]


@functools.lru_cache(maxsize=None)
def case_lp(name):
    """float64 log-probabilities [T, N, C] of a case."""
    return log_probs64(make_case(name).acts)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """The float64 reference of every utterance of a case: [(states or None, score)]."""
    k = make_case(name)
    lp = case_lp(name)
    return [viterbi(lp[:t, b], lab, k.blank) for b, t, lab in utterances(k)]


def rel_err(score, ref):
    return abs(score - ref) / max(abs(ref), 1.0)
