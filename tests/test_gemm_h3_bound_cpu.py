"""CPU: the fp16x3 GEMM's error model on the scale-edge inputs of test_gpu_gemm_contract.py,
without the kernel.

A NumPy emulation of the kernel's operand split (csrc/split_mma.h split_store8<2> with the
row scales of its h3_exp: fp16 hi and lo of the row-scaled value, the three products
hi*hi + hi*lo + lo*hi exact, scaled back) is compared with the float64 product under the bound
the GPU test asserts,

    |C - C64| <= 2^-20 (|A||B|) + 2^-38 (amax_A (x) sum_k |B| + sum_k |A| (x) amax_B),

which follows from the split: with claimed row maxima amax each staged element is off by at
most max(2^-22 |x|, 2^-39 amax) (hi and lo keep 11 bits each; lo's subnormal step 2^-24 sits
39 bits under the scaled maximum, 2^14 or more) and the dropped lo*lo term is below 2^-22 |ab|;
the bound doubles that.  So the inputs are shown to satisfy the bound before the kernel is
asked to.  This is an emulation, not a GPU measurement: its accumulator is float64.
"""
import numpy as np
import pytest

from gemm_common import (H3_CASES, bits_of, h3_bound, h3_case, h3_emulate, h3_exp, h3_maxima,
                         normal_range)


def test_h3_exp_matches_the_header():
    """split_mma.h h3_exp: the row's largest element lands in [2^14, 2^15); a zero, inf or NaN
    maximum keeps e = 0; the exponent clamps at 127 (2^e stays a normal float)."""
    x = np.array([1.0, 1.5, 2.0 ** -20, 65504.0, 2.0 ** 100, 0.0, np.inf, np.nan, 2.0 ** -120,
                  2.0 ** -149], dtype=np.float32)
    e = h3_exp(bits_of(x))
    assert list(e) == [14, 14, 34, -1, -86, 0, 0, 0, 127, 127]
    for v, ee in zip(x[:5], e[:5]):
        assert 2.0 ** 14 <= float(v) * 2.0 ** int(ee) < 2.0 ** 15


@pytest.mark.parametrize("name", H3_CASES)
def test_emulated_split_meets_the_bound(name):
    a, bt, a_claim, b_claim = h3_case(name)
    am, bm = h3_maxima(a, bt, a_claim, b_claim)
    assert (am >= np.abs(a).max(1)).all() and (bm >= np.abs(bt).max(1)).all()   # upper bounds
    ref = a.astype(np.float64) @ bt.astype(np.float64).T
    emu = h3_emulate(a, bt, bits_of(am), bits_of(bm))
    bound = h3_bound(a, bt, am, bm)
    keep = normal_range(ref)
    excluded = 1.0 - keep.mean()
    assert excluded < 0.01, excluded
    err = np.abs(emu - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))[keep].max()
        comp = np.where(err == 0, 0.0, err / (np.abs(a).astype(np.float64)
                                              @ np.abs(bt).astype(np.float64).T))[keep].max()
    print(f"{name}: emulation max err / bound {ratio:.4f}, componentwise {comp:.3e}, "
          f"excluded {excluded:.4%}")
    assert ratio <= 1.0, (name, ratio)
    if name == "zero":
        assert (emu[5, :] == 0).all() and (emu[:, 7] == 0).all()
    if name == "spike-24":
        # the documented limit: elements more than 2^17 below the row maximum lose bits, so
        # the plain componentwise error leaves the 1e-6 bar while staying inside the bound
        assert comp > 1e-6, comp
    if name in ("zero", "scaled-rows", "loose-0", "loose-8", "spike-10"):
        assert comp < 1e-6, comp
