"""CPU: the host side of the recurrent launch record (ds2_test_rnn_last_launch) and the
argument checks of the column-maxima entry points, none of which touches the GPU."""
import threading

from ds2amd import _lib, ops

INVALID_VALUE, UNSUPPORTED_SHAPE = 1, 2
PTR = 4096   # a non-null pointer the checks below never follow


def test_record_is_thread_local_and_starts_empty():
    seen = []
    th = threading.Thread(target=lambda: seen.append(ops.rnn_last_launch()))
    th.start()
    th.join()
    assert seen == [ops.RnnLaunch("none", 0, 0, 0, 0, 0, 0)]
    assert _lib.load().ds2_test_rnn_last_launch(None) == INVALID_VALUE


def test_column_maxima_decline_unaligned_columns_before_any_launch():
    """D H (RNN) or D 3H (GRU) no multiple of 4: the column pass that follows a kernel without
    the fused maxima could not run, so the entry points decline at once; the layers then call
    them without the maxima (test_unsorted_lengths_summed, one direction at H = 6)."""
    lib = _lib.load()
    for h, nd in ((6, 1), (7, 2)):
        rc = lib.ds2_rnn_bwd_ws(3, 2, h, nd, PTR, nd, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR,
                                1 << 20, None)
        assert rc == UNSUPPORTED_SHAPE
        rc = lib.ds2_gru_bwd_bias_amax(3, 2, h, nd, PTR, nd, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR,
                                       PTR, PTR, PTR, PTR, PTR, PTR, 1 << 20, None)
        assert rc == UNSUPPORTED_SHAPE
