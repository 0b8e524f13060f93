"""CPU: host-side contract of ds2_gru_row_amax (no launch: every case returns before HIP)."""
import ctypes

import torch  # noqa: F401  (load torch's HIP runtime first: one libamdhip64 per process)
from ds2amd import _lib


def test_row_amax_workspace_holds_the_partials():
    """The workspace with room for the row-maximum partials: the plain backward workspace plus
    [T N][D][H / 32] floats; 0 for invalid shapes."""
    base = _lib.size("ds2_gru_bwd_workspace_size", 32, 800, 2)
    big = _lib.size("ds2_gru_row_amax_workspace_size", 501, 32, 800, 2)
    assert big >= base + 501 * 32 * 2 * 25 * 4
    assert big < base + 501 * 32 * 2 * 25 * 4 + 4096
    assert _lib.size("ds2_gru_row_amax_workspace_size", 0, 32, 800, 2) == base
    assert _lib.size("ds2_gru_row_amax_workspace_size", 501, 32, 800, 3) == 0


def test_row_amax_status_without_partials():
    """A workspace no XCD-local backward has written partials into answers
    DS2_UNSUPPORTED_SHAPE (the caller's cue for ds2_amax), never a launch; bad arguments are
    DS2_INVALID_VALUE; an empty problem is DS2_OK."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    ws = ctypes.addressof(buf)
    assert lib.ds2_gru_row_amax(29, 7, 96, 1, ws, 1 << 30, ws, None) == _lib.UNSUPPORTED_SHAPE
    assert not _lib.call_or_unsupported("ds2_gru_row_amax", 29, 7, 96, 1, ws, 1 << 30, ws, None)
    assert lib.ds2_gru_row_amax(29, 7, 96, 3, ws, 1 << 30, ws, None) == 1
    assert lib.ds2_gru_row_amax(29, 7, 96, 1, None, 0, ws, None) == 1
    assert lib.ds2_gru_row_amax(29, 7, 96, 1, ws, 1 << 30, None, None) == 1
    assert lib.ds2_gru_row_amax(0, 7, 96, 1, None, 0, None, None) == 0
