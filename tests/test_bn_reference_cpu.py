"""CPU: what tests/test_gpu_bn.py takes for granted about its own cases (bn_common), asserted
on the float64 references alone.  A later change of a seed or a distribution that would make
the GPU comparison ambiguous (a value on a clamp edge) or hollow (a clamp side never taken, a
"stress" case that does not stress) fails here, without a GPU."""
import pytest
import torch

import bn_common as bc


@pytest.mark.parametrize("case", bc.PLANES_CASES, ids=bc.planes_id)
def test_planes_case_keeps_its_margin_from_the_clamp_bounds(case):
    """No unmasked pre-clamp value within CLAMP_MARGIN (2e-4, ~20 x the fp32 rounding of a value
    <= 40 through the apply's four operations) of 0 or 20: HIP and float64 then agree on which
    elements the Hardtanh passes, and the gradient is compared with no exclusions.  Cases with
    more than 500 unmasked values put at least 5 % of them on each clamp side."""
    _, r64, _ = bc.planes_case(*case)
    r = r64[0]
    u = r["pre"][r["unmasked"]]
    assert u.numel() > 0
    dist = torch.minimum((u - bc.LO).abs(), (u - bc.HI).abs()).min().item()
    lo = (u <= bc.LO).double().mean().item()
    hi = (u >= bc.HI).double().mean().item()
    print(f"{bc.planes_id(case)}: {u.numel()} unmasked, nearest to a bound {dist:.2e}, "
          f"<= 0: {lo:.3f}, >= 20: {hi:.3f}")
    assert dist >= bc.CLAMP_MARGIN
    if u.numel() > bc.CLAMP_SHARE_FROM:
        assert lo >= bc.CLAMP_SHARE and hi >= bc.CLAMP_SHARE
    # the pre-clamp values do not depend on dy's layout
    assert torch.equal(r64[1]["pre"], r["pre"])
    # masked positions: output and gradient exactly 0 in the reference too
    for layout in (0, 1):
        assert not r64[layout]["y"][~r["unmasked"]].any()
        assert not r64[layout]["dz"][~r["unmasked"]].any()


def test_planes_cases_reach_what_they_are_listed_for():
    """The shapes' reasons, restated as arithmetic on the kernels' constants (bn.hip:
    kPlaneSplit 4, BA_ROWS 4, 64 x 64 tiles, 256 threads)."""
    shapes = {bc.planes_id(c): c for c in bc.PLANES_CASES}
    n, c, d, t, lens, _ = shapes["3x5x5x70"]
    assert 64 % d and c * d < 64 and 0 in lens              # a 64-row f tile straddles channels
    n, c, d, t, lens, _ = shapes["2x3x1x257"]
    assert d == 1 and t == 257 and max(lens) > t
    n, c, d, t, lens, _ = shapes["4x2x3x64"]
    assert d < 4 and d % 2 == 1 and t == 64 and {0, 1, t - 1, t} <= set(lens)
    n, c, d, t, lens, _ = shapes["2x7x9x65"]
    assert d % 4 == 1 and t == 65 and c * d == 63
    n, c, d, t, lens, _ = shapes["2x32x2x600"]
    assert c == 32 and d * t == 2 * 512 + 176
    assert shapes["3x4x1x1"][2:4] == (1, 1) and 0 in shapes["3x4x1x1"][4]


@pytest.mark.parametrize("r,c,seed", bc.BN_RELU_CASES)
def test_bn_relu_case_keeps_its_margin_from_zero(r, c, seed):
    """No pre-ReLU value within RELU_MARGIN (1e-5, ~5 x the fp32 rounding of a value <= 10
    through the apply) of 0: the stored output's sign, which the backward reads, is the
    reference's at every element."""
    _, r64, _ = bc.rows_case(r, c, seed, "std", True)
    dist = r64["pre"].abs().min().item()
    share = (r64["pre"] > 0).double().mean().item()
    print(f"bn_relu {r}x{c}: nearest to 0 {dist:.2e}, active {share:.3f}")
    assert dist >= bc.RELU_MARGIN
    assert 0.2 < share < 0.8


@pytest.mark.parametrize("r,c", bc.OFFSET_SHAPES)
def test_offset_mean_case_stresses_the_mean_rounding(r, c):
    """x = 1000 + 0.01 randn: the float32 CPU reference is >= 1e-4 from float64 in y (the
    fp32-rounded mean against a spread of 0.01), so a HIP y inside bound(d32) and a HIP dx /
    dgamma inside the standard bounds say something about where the kernel keeps fp64."""
    case = bc.rows_case(r, c, 0, "off1000")
    ds = {k: bc.d32(case, k) for k in bc.ROWS_TENSORS}
    print(f"off1000 {r}x{c}: " + " ".join(f"{k} {v:.2e}" for k, v in ds.items()))
    assert ds["y"] >= 1e-4


def test_rows_shapes_meet_both_kernels_at_every_chunk_depth():
    """Every R whose chunks reach the two-rows-in-flight loop (per = ceil(R / 256) >= 5) meets a
    float4 and a scalar C; every C meets at least two R; R = 2 (dx analytically ~0) is absent."""
    per = lambda r: -(-r // 256)                                       # noqa: E731
    assert sorted({per(r) for r, _ in bc.ROWS_SHAPES}) == [1, 2, 5, 8, 9, 13]
    for r in {r for r, _ in bc.ROWS_SHAPES if per(r) >= 5}:
        cs = [c for rr, c in bc.ROWS_SHAPES if rr == r]
        assert any(c % 4 == 0 for c in cs) and any(c % 4 for c in cs), r
    for c in (4, 64, 260, 1, 3, 65, 130):
        assert len([r for r, cc in bc.ROWS_SHAPES if cc == c]) >= 2, c
    assert all(r != 2 for r, _ in bc.ROWS_SHAPES)


def test_references_start_from_the_float32_bits():
    """The float64 reference's input is the float32 draw, bit for bit, and b's zero-valued term
    leaves z's bits alone while still carrying b's gradient."""
    case = bc.PLANES_CASES[0]
    inp, r64, _ = bc.planes_case(*case)
    assert inp["z"].dtype == torch.float32
    m = bc.time_mask(case[4], case[3])
    assert torch.equal(inp["z"], (inp["z0"] + inp["b"][None, :, None, None]).masked_fill(m, 0))
    db = r64[0]["db"]
    assert torch.allclose(db, r64[0]["dz"].sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    assert db.abs().max().item() > 1e-3
