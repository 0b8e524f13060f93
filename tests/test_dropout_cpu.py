"""CPU: the host Philox4x32-10 the dropout tests use as their reference (known answers, the
dropped fraction of its mask) and the argument checks of the dropout entry points, which
return before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

import torch  # noqa: F401  (load torch's HIP runtime first: one libamdhip64 per process)
from ds2amd import _lib

import dropout_common as dc

OK, INVALID = 0, 1

# counter, key, output: the Random123 known-answer vectors of philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    got = dc.philox4x32_10([np.array([v]) for v in ctr], key)
    assert tuple(int(v[0]) for v in got) == out


def test_words_follow_the_header_mapping():
    """word j of the call with counter (g, 0, offset_lo, offset_hi) decides element 4 g + j"""
    w = dc.words(11, dc.SEED, (3 << 32) | 12)
    for i in (0, 5, 10):
        one = dc.philox4x32_10([np.array([i // 4]), np.array([0]), np.array([12]), np.array([3])],
                               (dc.SEED & dc.MASK32, dc.SEED >> 32))
        assert int(w[i]) == int(one[i % 4][0])
    assert dc.threshold(0.5) == 1 << 31 and dc.threshold(0.0) == 0
    assert dc.threshold(0.2) == math.floor(float(np.float32(0.2)) * 2.0 ** 32)


@pytest.mark.parametrize("p", [0.2, 0.5, 0.05])
def test_dropped_fraction_within_5_sigma(p):
    n = 1 << 20
    frac = 1.0 - dc.keep_mask((n,), p, dc.SEED, dc.OFFSET).mean()
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"p {p}: dropped {frac:.6f}, {abs(frac - p) / sigma:.2f} sigma")
    assert abs(frac - p) <= 5 * sigma


A = 256     # a non-NULL, 16-byte aligned address that is never dereferenced


def _apply(rows, c, p):
    return _lib.load().ds2_dropout_apply(A, rows, c, p, dc.SEED, dc.OFFSET, A, None)


def _fused(rows, c, p, relu=1):
    return _lib.load().ds2_bn_dropout_apply_amax(A, rows, c, A, A, A, A, relu, p, dc.SEED,
                                                 dc.OFFSET, A, A, A, None)


def _bwd(rows, c, p):
    return _lib.load().ds2_bn_relu_dropout_bwd(A, A, A, rows, c, A, A, A, A, p, A, A, A, A,
                                               1 << 20, None)


@pytest.mark.parametrize("call", [_apply, _fused, _bwd])
def test_arguments_checked_without_a_launch(call):
    for p in (-0.1, 1.5, float("nan")):
        assert call(4, 8, p) == INVALID, p
    assert call(-1, 8, 0.2) == INVALID
    assert call(4, -4, 0.2) == INVALID
    assert call(0, 8, 0.2) == OK
    assert call(4, 0, 0.2) == OK
    # a bad p is reported even where nothing would be launched
    assert call(0, 8, 1.5) == INVALID


def test_prototypes_take_64_bit_seed_and_offset():
    for name, at in (("ds2_dropout_apply", (4, 5)), ("ds2_bn_dropout_apply_amax", (9, 10))):
        argtypes = _lib._PROTOS[name][1]
        assert all(argtypes[i] is ctypes.c_uint64 for i in at), name
