"""CPU: the shape table of the Conv1d contract tests (conv1d_common.CASES, run on the GPU by
test_gpu_conv1d_contract.py) reaches every path of the dispatch (csrc/conv1d.hip c1_plan) and
every tile, stage-count, slab and loader edge it is there for, by the library's own plan.
Host queries only."""
import pytest

import torch  # noqa: F401  (load torch's HIP runtime first: one libamdhip64 per process)
from ds2amd import _lib, ops

from conv1d_common import (CASES, DIRS, GEMM, GEN, H3, SCALAR, SETTINGS, VEC, case_settings, out_len,
                           plan, plans, query, ref64, set_env, want_paths)


@pytest.mark.parametrize("case,setting", case_settings())
def test_the_plan_gives_the_path_the_table_claims(monkeypatch, case, setting):
    set_env(monkeypatch, setting)
    got = plans(CASES[case].cfg)
    assert tuple(got[d].path for d in DIRS) == want_paths(case, setting), (case, setting, got)


def test_the_table_reaches_every_path():
    """A path added to ops.CONV1D_PATHS without a contract case fails here ("none": the empty
    calls below)."""
    have = {p for c in CASES.values() for p in c.paths}
    assert have == set(ops.CONV1D_PATHS) - {"none"}
    for cfg in ((0, 2, 32, 32, 3, 1, 1), (9, 0, 32, 32, 3, 1, 1)):
        assert all(pl.path == "none" and pl.ws_bytes == 0 for pl in plans(cfg).values())


def _default_plans():
    return {(c, d): pl for c, case in CASES.items() for d, pl in plans(case.cfg).items()}


def test_the_table_reaches_every_stage_count_edge(monkeypatch):
    """CFLUSH = 8: a flush inside the loop happens after stages 8, 16, ...; the final flush
    takes what is left.  Below 8 (only the final flush), 8n + 1 and 8n + 2 (a final flush of
    one and two stages), and a multiple of 8 (a final flush of nothing)."""
    set_env(monkeypatch, "default")
    st = {pl.stages for pl in _default_plans().values() if pl.path in (VEC, SCALAR)}
    assert any(0 < v < 8 for v in st), st
    assert any(v > 8 and v % 8 == 1 for v in st), st
    assert any(v > 8 and v % 8 == 2 for v in st), st
    assert any(v >= 8 and v % 8 == 0 for v in st), st
    # the stage counts the table names
    p = _default_plans()
    assert [p[c, "fwd"].stages for c in "ABCDK"] == [78, 10, 4, 4, 9]
    assert (p["B", "dgrad"].stages, p["F1", "fwd"].stages, p["R", "fwd"].stages) == (25, 2, 248)


def test_the_table_reaches_every_tile_and_slab_edge(monkeypatch):
    set_env(monkeypatch, "default")
    p = _default_plans()
    ig = [pl for pl in p.values() if pl.path in (VEC, SCALAR)]
    wg = [pl for pl in p.values() if pl.path == H3]
    for group in (ig, wg):
        assert any(pl.gx > 1 and pl.gy > 1 for pl in group)
    # more than one slab, the last one no multiple of 32 rows
    rows = {c: out_len(CASES[c].cfg) * CASES[c].cfg[1] for c in CASES}
    last = {c: rows[c] - (pl.nsplit - 1) * pl.kchunk for (c, d), pl in p.items()
            if d == "wgrad" and pl.path == H3 and pl.nsplit > 1}
    assert any(v % 32 for v in last.values()), last
    assert all(0 < v <= p[c, "wgrad"].kchunk for c, v in last.items())
    # every slab but the last is whole 32-row stages: c1_wgrad_kernel's `r < kend` then cuts only
    # the last slab, at the end of the rows (why replacing it by `r < R` changes nothing)
    for (c, d), pl in p.items():
        if pl.path == H3:
            assert pl.kchunk % 32 == 0 and (pl.nsplit - 1) * pl.kchunk < rows[c] <= pl.nsplit * pl.kchunk
    i = p["I", "wgrad"]
    assert (i.nsplit, i.kchunk, i.gz, last["I"]) == (4, 256, 4, 135)
    # what the table says of single cases
    assert (p["A", "wgrad"].gx, p["B", "wgrad"].gy, p["R", "fwd"].gx, p["I", "fwd"].gy) == (17, 2, 3, 8)
    assert p["L", "fwd"].gy == 1 and rows["L"] == 128
    assert p["B", "fwd"].gy == 2 and rows["B"] == 135
    # the grid-stride kernels' second iteration: more than 8192 * 256 elements
    t, n, ci, co, k, s, pd = CASES["R"].cfg
    assert co * k * ci > 8192 * 256 and ci * k * ((co + 31) // 32 * 32) > 8192 * 256


def test_the_scalar_loader_is_reached_by_channel_count_and_by_address(monkeypatch):
    set_env(monkeypatch, "default")
    assert CASES["A"].cfg[2] % 4 != 0 and plan("fwd", CASES["A"].cfg, 0).path == SCALAR
    assert CASES["B"].cfg[3] % 4 != 0 and plan("dgrad", CASES["B"].cfg, 0).path == SCALAR
    for c, d in (("B", "fwd"), ("I", "fwd"), ("I", "dgrad")):
        assert plan(d, CASES[c].cfg, 0x1000).path == VEC
        for low in (4, 8, 12):
            assert plan(d, CASES[c].cfg, 0x1000 + low).path == SCALAR, (c, d, low)


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_plan_never_asks_for_more_than_the_query(monkeypatch, setting):
    set_env(monkeypatch, setting)
    for c, case in CASES.items():
        for d, pl in plans(case.cfg).items():
            assert pl.ws_bytes <= query(d, case.cfg), (c, d, pl.ws_bytes, query(d, case.cfg))
            assert (pl.ws_bytes == 0) == (d != "wgrad" and pl.path in (GEN, GEMM)), (c, d, pl)


def test_supplied_maxima_save_one_pass(monkeypatch):
    set_env(monkeypatch, "default")
    for c in ("B", "I"):
        for d in ("fwd", "wgrad"):
            assert (plan(d, CASES[c].cfg).amax_passes, plan(d, CASES[c].cfg, amax_given=True).amax_passes) == (2, 1)
    set_env(monkeypatch, "general")
    assert all(plan(d, CASES["B"].cfg, amax_given=g).amax_passes == 0 for d in DIRS for g in (False, True))


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("cfg", [(4, 2, 8, 8, 13, 1, 2), (4, 2, 8, 8, 14, 2, 4), (4, 2, 32, 32, 13, 1, 2),
                                 (4, 2, 32, 32, 14, 2, 4)])
def test_a_kernel_longer_than_the_padded_input_is_invalid(monkeypatch, setting, cfg):
    """T + 2p - k = -1 and -2: no output row at stride 1 or 2 (a division that truncates toward
    zero gives (-1) / 2 + 1 = 1 row)."""
    set_env(monkeypatch, setting)
    for d in DIRS:
        with pytest.raises(_lib.Ds2Error, match="DS2_INVALID_VALUE"):
            plan(d, cfg)
        assert query(d, cfg) == 0


def test_the_plan_rejects_what_the_entry_points_reject():
    good = (10, 2, 32, 32, 3, 1, 1)
    for i, v in ((0, -1), (1, -2), (2, 0), (3, 0), (4, 0), (5, 0), (6, -1)):
        bad = good[:i] + (v,) + good[i + 1:]
        for d in DIRS:
            with pytest.raises(_lib.Ds2Error, match="DS2_INVALID_VALUE"):
                plan(d, bad)
    for d in DIRS:                      # Cout Cin k = 2^31
        with pytest.raises(_lib.Ds2Error, match="DS2_UNSUPPORTED_SHAPE"):
            plan(d, (10, 2, 1 << 15, 1 << 15, 2, 1, 1))
    lib = _lib.load()
    assert lib.ds2_test_conv1d_plan(3, *good, 0, None) == 1      # no such direction
    assert lib.ds2_test_conv1d_plan(0, *good, 0, None) == 1      # nowhere to write the plan


def test_the_componentwise_bound_has_room_over_an_independent_float32():
    """conv1d_common.COMP_REL = 2e-6 is meant as 8 x what float32 torch on the CPU needs against
    float64 on the same inputs (2.5e-7 when the table was made); another CPU may sum in another
    order, so only half of that room is asserted."""
    worst = max(v for c in CASES.values() for v in ref64(c.cfg).cpu32.values())
    print(f"float32 CPU torch, worst componentwise ratio over the table: {worst:.3e}")
    assert worst <= 5e-7
