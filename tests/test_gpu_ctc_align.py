"""ds2_ctc_align (csrc/ctc.hip: log-softmax, prep, the max-plus scan with back-pointers, the
chunked back-trace) against the float64 dynamic programme of ctc_align_common, at the shapes
where the kernel's code paths change (ctc_align_common._CASES names them).

Every feasible utterance is checked for validity (a monotone path with legal steps, start and
end, frame labels that collapse to the target, spans that agree with the states, a -1 tail),
the exact float64 path, the score within 1e-6 * max(|ref|, 1), and optimality: the float64
score of the returned path is at least ref - 2e-6 * max(|ref|, 1) (the kernel maximises a score
that is itself within 1e-6 relative of the true one).  An infeasible utterance has score -inf
and -1 in all of its states and spans.  test_ctc_align_cpu.py shows that float32 decides no
comparison of these inputs differently from float64, so the exact path is a fair demand.
"""
import numpy as np
import pytest
import torch

import ctc_align_common as ac
from ds2amd import _lib, ops

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------- helpers
def _raw(dev, k, max_l=None):
    max_l = int(k.label_lens.max()) if max_l is None else max_l
    states, spans, scores = ops.ctc_align_raw(k.acts.to(dev), k.labels.to(dev),
                                              k.act_lens.to(dev), k.label_lens.to(dev), max_l,
                                              blank=k.blank)
    torch.cuda.synchronize()
    return states.cpu(), spans.cpu(), scores.cpu()


def _check_case(tag, k, lp, ref, states, spans, scores):
    """The four checks of the module docstring on every utterance; returns the worst score
    error and optimality gap (relative)."""
    t_max = k.acts.shape[0]
    assert states.shape == (len(k.per_sample), t_max) and states.dtype == torch.int32
    assert spans.shape == (int(k.label_lens.sum()), 2)
    worst, gap = 0.0, 0.0
    off = 0
    for (b, t, lab), (ref_states, ref_score) in zip(ac.utterances(k), ref):
        row = states[b].tolist()
        sp = spans[off:off + len(lab)].tolist()
        off += len(lab)
        score = float(scores[b])
        where = (tag, b)
        if ref_states is None:
            assert score == float("-inf"), where
            assert row == [-1] * t_max, where
            assert sp == [[-1, -1]] * len(lab), where
            continue
        got = row[:t]
        # 1. validity
        assert row[t:] == [-1] * (t_max - t), where
        assert ac.validity_errors(got, lab, k.blank) == [], where
        assert sp == ac.spans_of(got, len(lab)), where
        # 2. the exact path
        assert got == ref_states, where
        # 3. the score
        err = ac.rel_err(score, ref_score)
        assert err <= ac.COST_RTOL, (where, score, ref_score)
        # 4. optimality of the returned path in float64
        g = (ref_score - ac.path_score64(lp[:t, b], got, lab, k.blank)) / max(abs(ref_score), 1.0)
        assert g <= 2 * ac.COST_RTOL, (where, g)
        worst, gap = max(worst, err), max(gap, g)
    print(f"ctc_align[{tag}]: score rel err {worst:.2e}, optimality gap {gap:.2e}")
    return worst, gap


# ---------------------------------------------------------------------------- 1. the matrix
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_align_matrix_vs_fp64(dev, name):
    """ops.ctc_align_raw on every case of ctc_align_common._CASES: validity, the exact float64
    path, score and optimality per utterance; a second call is bit-identical."""
    k = ac.make_case(name)
    out = _raw(dev, k)
    _check_case(name, k, ac.case_lp(name), ac.case_ref(name), *out)
    again = _raw(dev, k)
    for a, b in zip(out, again):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- 2. named cases
def test_align_degenerate_batch(dev):
    """L = 0: every state 0 and the score the sum of the blank's log-probabilities; T = 0 with
    L = 0: score 0; T = 0 with L = 2 and T = need - 1: -inf and -1 next to feasible neighbours;
    T = need with repeats: the single path whatever the logits; act_len > t_max is clamped."""
    k = ac.make_case("degenerate")
    lp = ac.case_lp("degenerate")
    states, spans, scores = _raw(dev, k)
    assert states[0].tolist() == [0] * 12
    blank_sum = lp[:, 0, k.blank].sum()
    assert abs(float(scores[0]) - blank_sum) <= ac.COST_RTOL * abs(blank_sum)
    assert float(scores[1]) == 0.0 and states[1].tolist() == [-1] * 12
    assert float(scores[2]) == float("-inf") and float(scores[3]) == float("-inf")
    assert spans[:2].tolist() == [[-1, -1]] * 2 and spans[2:7].tolist() == [[-1, -1]] * 5
    assert states[4].tolist() == [1, 2, 3, 5, 6, 7, 8, 9, -1, -1, -1, -1]
    assert spans[7:12].tolist() == [[0, 1], [2, 3], [3, 4], [5, 6], [7, 8]]
    assert states[5, 7:].tolist() == [-1] * 5 and int(states[5, 6]) >= 5
    assert int(states[6].min()) >= 0                      # all 12 frames of the clamped row
    # the single path does not depend on the logits
    other = ac._case(170, 12, 6, k.act_lens.tolist(), None, labels=k.per_sample)
    assert _raw(dev, other)[0][4].tolist() == states[4].tolist()


def test_align_tie_rule_on_zero_logits(dev):
    """All-zero logits: every alignment has the same score in float32 too, so the path is the
    tie rule's alone (stay, then s - 1, then s - 2, strictly greater; S - 1 at the end unless
    S - 2 is greater) -- over 140 frames: two back-trace chunks and 17 rescalings."""
    k, lp, ref = ac.ties_long()
    _check_case("ties_long", k, lp, ref, *_raw(dev, k))


def test_align_planted_path_comes_back(dev):
    """0.1 noise and +12 along a drawn valid alignment: exactly that alignment is returned."""
    k, planted = ac._planted(84, 140, 30, 29)
    states, spans, _ = _raw(dev, k)
    assert states[0].tolist() == planted
    assert spans.tolist() == ac.spans_of(planted, 30)


def test_align_wider_rows_than_the_labels(dev):
    """max_label_len above every label length only widens the back-pointer rows: same
    outputs."""
    k = ac.make_case("bp_chunk_edges")
    base = _raw(dev, k)
    wide = _raw(dev, k, max_l=333)
    for a, b in zip(base, wide):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- 3. contract
def test_align_argument_contract(dev):
    """The status codes of ds2_ctc_loss, returned before any launch: max_label_len = 1025 is
    DS2_UNSUPPORTED_SHAPE, c = 65 and a blank outside [0, c) DS2_INVALID_VALUE, a short or
    missing workspace DS2_WORKSPACE_TOO_SMALL, n = 0 DS2_OK.  The output buffers keep their
    canary, so nothing ran."""
    lib = _lib.load()
    t, n, c, max_l = 10, 2, 6, 3
    acts = torch.zeros(t, n, 65, device=dev)
    labels = torch.ones(6, dtype=torch.int32, device=dev)
    lens = torch.full((n,), 3, dtype=torch.int32, device=dev)
    act_lens = torch.full((n,), t, dtype=torch.int32, device=dev)
    states = torch.full((n, t), 77, dtype=torch.int32, device=dev)
    spans = torch.full((6, 2), 77, dtype=torch.int32, device=dev)
    scores = torch.full((n,), 77.0, device=dev)
    need = _lib.size("ds2_ctc_align_workspace_size", t, n, max_l)
    assert need >= n * t * c * 4 + n * t * (2 * max_l + 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(n_=n, c_=c, max_l_=max_l, blank=0, ws_ptr=ws.data_ptr(), ws_bytes=need):
        return lib.ds2_ctc_align(acts.data_ptr(), t, n_, c_, labels.data_ptr(), lens.data_ptr(),
                                 act_lens.data_ptr(), max_l_, blank, states.data_ptr(),
                                 spans.data_ptr(), scores.data_ptr(), ws_ptr, ws_bytes, None)

    assert call(max_l_=1025) == 2
    assert call(c_=65) == 1 and call(c_=0) == 1
    assert call(blank=6) == 1 and call(blank=-1) == 1 and call(n_=-1) == 1
    assert call(ws_bytes=need - 1) == 5 and call(ws_ptr=None) == 5
    assert call(n_=0) == 0 and call(n_=0, ws_ptr=None, ws_bytes=0) == 0
    torch.cuda.synchronize()
    assert (states == 77).all() and (spans == 77).all() and (scores == 77.0).all()
    with pytest.raises(_lib.Ds2Error):
        ops.ctc_align_raw(acts, labels, act_lens, lens, max_l)          # c = 65
    with pytest.raises(_lib.Ds2Error):
        ops.ctc_align_raw(acts.cpu()[:, :, :6], labels, act_lens, lens, max_l)
    assert call() == 0                                                   # and the real call runs
    torch.cuda.synchronize()
    assert not (states == 77).any()


# ---------------------------------------------------------------------------- 4. Python surface
def test_forced_align_result_object(dev):
    """ds2amd.ctc.forced_align with host labels and lengths: states and scores are the raw
    op's, frame_labels the label per frame (-1 beyond the length and for an infeasible
    utterance), spans split per utterance; host labels outside [0, C) are a ValueError."""
    from ds2amd.ctc import forced_align
    k = ac.make_case("degenerate")
    states, spans, scores = _raw(dev, k)
    res = forced_align(k.acts.to(dev), k.labels, k.act_lens, k.label_lens, blank=k.blank)
    assert torch.equal(res.states.cpu(), states) and torch.equal(res.scores.cpu(), scores)
    assert res.frame_labels.is_cuda and not res.states.requires_grad
    assert [int(s.shape[0]) for s in res.spans] == k.label_lens.tolist()
    assert torch.equal(torch.cat(res.spans).cpu(), spans)
    fl = res.frame_labels.cpu().tolist()
    for (b, t, lab), (ref_states, _) in zip(ac.utterances(k), ac.case_ref("degenerate")):
        if ref_states is None:
            assert fl[b] == [-1] * 12
        else:
            assert fl[b] == ac.frame_labels(ref_states, lab, k.blank) + [-1] * (12 - t)
    res_d = forced_align(k.acts.to(dev), k.labels.to(dev), k.act_lens.to(dev),
                         k.label_lens.to(dev), blank=k.blank)
    assert torch.equal(res_d.frame_labels, res.frame_labels)
    with pytest.raises(ValueError):
        forced_align(k.acts.to(dev), k.labels + 6, k.act_lens, k.label_lens)


def test_align_batch_end_to_end(dev):
    """A small seeded BiGRU DeepSpeech, two synthetic clips and their transcripts through
    ds2amd.transcribe.align_batch: the frame labels behind the returned spans equal the
    float64 reference applied to the model's own logits, chars and words tile the transcript,
    and a transcript longer than its clip's frames gives None."""
    from ds2amd import model as dsm
    from ds2amd.data_loader import SpectrogramParser
    from ds2amd.transcribe import align_batch, frame_to_seconds
    labels = "_'ABCDEFGHIJKLMNOPQRSTUVWXYZ2 "
    conf = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
    torch.manual_seed(11)
    m = dsm.DeepSpeech(rnn_type='gru', labels=labels, rnn_hidden_size=32, nb_layers=2,
                       audio_conf=conf, bidirectional=True).to(dev).eval()
    parser = SpectrogramParser(conf, normalize='max_frame', device=dev)
    rng = np.random.default_rng(5)
    clips = []
    for i, secs in enumerate([0.8, 0.5]):
        n = int(16000 * secs)
        y = 0.1 * rng.standard_normal(n) + np.sin(2 * np.pi * (300 + 200 * i) * np.arange(n) / 16e3)
        clips.append((y / np.abs(y).max()).astype(np.float32))
    texts = ["HELLO WORLD", "AB CD"]
    out = align_batch(clips, texts, parser, m, labels)
    with torch.no_grad():
        spect, frames = parser.parse_batch(clips)
        logits, _, out_lens = m(spect, frames)
    lp = ac.log_probs64(logits.cpu())                                  # [N, T, C]
    for b, (text, res) in enumerate(zip(texts, out)):
        ids = [labels.index(ch) for ch in text]
        t = int(out_lens[b])
        ref_states, ref_score = ac.viterbi(lp[b, :t], ids, 0)
        assert res is not None and ref_states is not None
        assert [ch for ch, _, _ in res['chars']] == list(text)
        assert [[s0, s1] for _, s0, s1 in res['chars']] == ac.spans_of(ref_states, len(ids))
        frames_of = [0] * t                      # the frame labels the spans stand for
        for i, (_, s0, s1) in zip(ids, res['chars']):
            frames_of[s0:s1] = [i] * (s1 - s0)
        assert frames_of == ac.frame_labels(ref_states, ids, 0)
        assert ac.rel_err(res['score'], ref_score) <= ac.COST_RTOL
        assert [w for w, _, _ in res['words']] == text.split()
        for (w, w0, w1), first in zip(res['words'], np.cumsum([0] + [len(x) + 1 for x in
                                                                    text.split()])):
            assert (w0, w1) == (res['chars'][first][1], res['chars'][first + len(w) - 1][2])
    too_long = align_batch(clips, ["HELLO WORLD", "AB CD " * 10], parser, m, labels)
    assert too_long[1] is None and too_long[0]['chars'] == out[0]['chars']
    assert frame_to_seconds(10, parser) == pytest.approx(0.2)
