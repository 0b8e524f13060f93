"""Shared by the dropout tests (not a test module): a host Philox4x32-10 in numpy and the
keep mask of include/ds2hip.h's mapping, written from the header alone --
    key = (seed_lo, seed_hi);  counter of group g = i // 4: (g_lo, g_hi, offset_lo, offset_hi);
    word i % 4 of that call decides element i;  dropped iff word < floor(p 2^32)
-- plus the float64 / float32 torch restatement of the Wav2Letter model with explicit masks."""
import numpy as np
import torch

import w2l_common as wc

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
SEED, OFFSET = 0x1234ABCD5678EF01, 8


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in ctr]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)
        p1 = c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0 = (k0 + W0) & MASK32
        k1 = (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def words(n, seed, offset):
    """the deciding uint32 word of each of n consecutive elements"""
    groups = (n + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    w = philox4x32_10((g & np.uint64(MASK32), g >> np.uint64(32),
                       np.full(groups, offset & MASK32, np.uint64),
                       np.full(groups, (offset >> 32) & MASK32, np.uint64)),
                      (seed & MASK32, (seed >> 32) & MASK32))
    return np.stack(w, axis=1).reshape(-1)[:n]


def keep_mask(shape, p, seed, offset):
    """bool array of `shape` (row-major): True where the element survives"""
    n = int(np.prod(shape))
    return (words(n, seed, offset).astype(np.uint64) >= np.uint64(threshold(p))).reshape(shape)


def scale32(p):
    """the survivors' factor as the kernels form it: 1.0f / (1.0f - p) in float32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def w2l_masked_forward(ref, x, masks, p):
    """wc.TorchW2L `ref` (any dtype) on x [N,1,161,T] with dropout after every block: masks[b]
    is block b's keep mask over the time-major [T' N][C] matrix the HIP forward sees.  Returns
    logits [N,T',C]."""
    dt = next(ref.parameters()).dtype
    sc = float(scale32(p))
    not_glu = any(isinstance(m, torch.nn.ReLU) for m in ref.rnns)
    last = torch.nn.ReLU if not_glu else torch.nn.BatchNorm1d
    h = x.squeeze(1).to(dt)
    b = 0
    for m in ref.rnns:
        h = m(h)
        if isinstance(m, last):
            n, c, t = h.shape
            k = torch.from_numpy(masks[b].reshape(t, n, c)).permute(1, 2, 0)
            h = h * (k.to(dt) * sc)
            b += 1
    assert b == len(masks)
    return ref.fc(h).transpose(1, 2)


def torch_w2l(form, dtype, layers):
    m = wc.TorchW2L(wc.FORMS[form], layers=layers, classes=len(wc.labels()))
    return m.to(dtype)
