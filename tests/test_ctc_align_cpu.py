"""CPU guards of the CTC forced-alignment tests: the float64 dynamic programme of
ctc_align_common against brute force, its float32 restatement (what the kernel computes)
against float64 on every case the GPU tests run, the ctypes prototypes, and the off-GPU
errors of the Python surface."""
import itertools

import numpy as np
import pytest
import torch

import ctc_align_common as ac
from ds2amd import _lib, ctc, transcribe


def test_dp_equals_brute_force_on_every_small_shape():
    """T <= 6, L <= 2, C = 3 (blank 0, then blank 1): the float64 dynamic programme returns
    the best of all C^T frame labellings that collapse to the target, and says 'does not fit'
    exactly when there is none."""
    gen = torch.Generator().manual_seed(90)
    n = 0
    for blank in (0, 1):
        classes = [c for c in range(3) if c != blank]
        targets = [[]] + [[a] for a in classes] + [list(p) for p in
                                                   itertools.product(classes, repeat=2)]
        for t in range(1, 7):
            lp = ac.log_probs64(torch.randn(t, 3, generator=gen) * 2)
            for lab in targets:
                frames, best = ac.brute_force(lp, lab, blank)
                states, score = ac.viterbi(lp, lab, blank)
                if frames is None:
                    assert states is None and score == -np.inf and ac.need(lab) > t
                    continue
                assert ac.validity_errors(states, lab, blank) == []
                assert ac.frame_labels(states, lab, blank) == frames, (t, lab, blank)
                assert abs(score - best) <= 1e-12 * max(abs(best), 1.0)
                n += 1
    assert n > 60
    assert ac.viterbi(np.zeros((0, 3)), [], 0) == ([], 0.0)
    assert ac.viterbi(np.zeros((0, 3)), [1], 0) == (None, -np.inf)


@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_float32_restatement_returns_the_float64_path(name):
    """On every case of the GPU matrix the float32 dynamic programme, unrescaled and rescaled
    every 8 rows as the kernel does, returns the float64 path exactly and a score within
    1e-6 * max(|ref|, 1): the inputs have no near-tie that float32 decides differently, so the
    GPU tests may ask for the exact path."""
    k = ac.make_case(name)
    lp = ac.case_lp(name)
    ref = ac.case_ref(name)
    worst = [0.0, 0.0]
    for (b, t, lab), (states, score) in zip(ac.utterances(k), ref):
        if states is None:
            assert ac.need(lab) > t
        else:
            assert ac.need(lab) <= t
            assert ac.validity_errors(states, lab, k.blank) == []
            assert abs(ac.path_score64(lp[:t, b], states, lab, k.blank) - score) <= \
                1e-9 * max(abs(score), 1.0)
        for i, rescale in enumerate((0, ac.RESCALE)):
            s32, sc32 = ac.viterbi(lp[:t, b], lab, k.blank, np.float32, rescale)
            assert s32 == states, (name, b, rescale)
            if states is not None:
                err = ac.rel_err(sc32, score)
                worst[i] = max(worst[i], err)
                assert err <= ac.COST_RTOL, (name, b, rescale, err)
    print(f"ctc_align[{name}]: fp32 score rel err {worst[0]:.2e} unrescaled, "
          f"{worst[1]:.2e} rescaled")


def test_long_tie_case_float32_path_and_rescaled_score():
    """ties_long (all-zero logits, T = 140 / 130): float32 returns the float64 path with and
    without rescaling; the score bound holds for the rescaled sum, which is what the kernel
    computes (the unrescaled one drifts, see ties_long)."""
    k, lp, ref = ac.ties_long()
    for (b, t, lab), (states, score) in zip(ac.utterances(k), ref):
        assert ac.validity_errors(states, lab, k.blank) == []
        for rescale in (0, ac.RESCALE):
            s32, sc32 = ac.viterbi(lp[:t, b], lab, k.blank, np.float32, rescale)
            assert s32 == states
        assert ac.rel_err(sc32, score) <= ac.COST_RTOL


def test_cases_cover_what_they_claim():
    """The shapes the kernel's constants ask for are in the matrix, and the degenerate batch
    holds an infeasible utterance, a single-path one and both empty kinds."""
    deg = ac.case_ref("degenerate")
    k = ac.make_case("degenerate")
    assert [s is None for s, _ in deg] == [False, False, True, True, False, False, False]
    assert deg[1] == ([], 0.0)
    assert deg[0][0] == [0] * 12
    assert abs(deg[0][1] - ac.case_lp("degenerate")[:, 0, k.blank].sum()) < 1e-12
    assert deg[4][0] == [1, 2, 3, 5, 6, 7, 8, 9]          # the only path of 2 2 3 3 3 in 8
    assert len(deg[6][0]) == 12                            # act_len 20 clamped to t_max
    assert ac.make_case("ownership").label_lens.tolist() == [255, 256, 257]
    assert ac.make_case("full_states").label_lens.tolist() == [1024]
    assert ac.make_case("bp_chunk_edges").act_lens.tolist() == [ac.BP_CHUNK - 1, ac.BP_CHUNK,
                                                                ac.BP_CHUNK + 1]
    assert len(ac.make_case("many_utts").per_sample) == 65
    assert (ac.make_case("c64_blank63").labels == 62).any()
    assert ac.make_case("ties").acts.count_nonzero().item() == 0
    planted, states = ac._planted(84, 140, 30, 29)
    assert ac.validity_errors(states, planted.per_sample[0].tolist()) == []
    assert ac.case_ref("planted")[0][0] == states


def test_protos_hold_the_alignment_symbols():
    for name in ("ds2_ctc_align_workspace_size", "ds2_ctc_align"):
        assert name in _lib._PROTOS, name
    assert len(_lib._PROTOS["ds2_ctc_align"][1]) == 15


def test_python_surface_raises_off_the_gpu():
    acts = torch.randn(5, 1, 4)
    with pytest.raises(RuntimeError):
        ctc.forced_align(acts, torch.tensor([1, 2], dtype=torch.int32), torch.tensor([5]),
                         torch.tensor([2]))

    class _Parser(object):            # never reached: the model's device is checked first
        window_stride = 0.01
        channel = -1

    with pytest.raises(RuntimeError):
        transcribe.align_batch([np.zeros(1600, dtype=np.float32)], ["AB"], _Parser(),
                               torch.nn.Linear(2, 2), "_AB ")
