"""CPU: the shape table of the Conv2d contract tests (conv_common.CASES, run on the GPU by
test_gpu_conv_contract.py) reaches every rung of the dispatch, every conv1_patch_fwd_kernel
instance and every conv_wgrad_patch_kernel form.  Host queries only."""
import pytest

import torch  # noqa: F401  (load torch's HIP runtime first: one libamdhip64 per process)
from ds2amd import _lib, ops

from conv_common import ALL_CASES, DIRS, SETTINGS, case_settings, plans, rung_name, set_env, table_rungs


@pytest.mark.parametrize("case,setting", case_settings(ALL_CASES))
def test_the_plan_gives_the_rung_the_table_claims(monkeypatch, case, setting):
    set_env(monkeypatch, setting)
    cfg, rungs = ALL_CASES[case]
    got = plans(cfg)
    for d, want in zip(DIRS, rungs[setting]):
        assert want is None or rung_name(got[d]) == want, (case, setting, d, rung_name(got[d]))


@pytest.mark.parametrize("cfg", [(2, 4, 9, 20, 8, 12, 3, 2, 1, 1, 1), (2, 4, 9, 20, 8, 3, 23, 2, 2, 1, 1),
                                 (2, 4, 9, 20, 8, 12, 3, 1, 1, 1, 1), (2, 4, 9, 20, 8, 3, 23, 2, 1, 1, 1)])
def test_a_kernel_larger_than_the_padded_input_is_invalid(cfg):
    """h + 2 ph - kh = -1 (or the same in w): no output row, whatever the stride (a division
    that truncates toward zero gave one at stride 2)."""
    with pytest.raises(_lib.Ds2Error, match="DS2_INVALID_VALUE"):
        plans(cfg)
    assert _lib.size("ds2_conv2d_workspace_size", *cfg) == 0
    assert _lib.size("ds2_conv2d_wgrad_workspace_size", *cfg) == 0


def test_every_case_names_all_three_default_rungs_or_is_forward_only():
    for name, case in ALL_CASES.items():
        assert set(case.rungs) <= set(SETTINGS), name
        d = case.rungs["default"]
        assert all(d) or (d[0] and not d[1] and not d[2]), name


def test_the_table_reaches_every_rung_and_instance():
    """A rung added to ops.CONV_RUNGS without a contract case fails here."""
    want = {r for r in ops.CONV_RUNGS if r not in ("none", "fwd_c1", "wg_patch")}
    want |= {f"fwd_c1:{a}" for a in (2, 3, 4, 5, 6)}
    want |= {f"wg_patch:{a}:{b}" for a in (2, 4) for b in (1, 2)}
    have = table_rungs()
    assert have == want, (sorted(want - have), sorted(have - want))
