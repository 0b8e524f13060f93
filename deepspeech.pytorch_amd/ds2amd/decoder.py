"""Decoders — drop-in for the reference ``decoder.py``.

``GreedyDecoder.decode`` runs argmax + CTC collapse in one HIP kernel
(ds2_greedy_decode) and copies back only the compacted label ids/offsets, instead
of the reference's per-frame ``.item()`` loop (ref decoder.py:165-197).  The
string semantics are the reference's: first maximum wins, blanks dropped, a
frame equal to the previous *frame* is dropped, the space label maps to ' ' and
'2' is emitted literally.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


def _levenshtein(a, b) -> int:
    """Edit distance (python-Levenshtein's Lev.distance semantics)."""
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


class Decoder(object):
    """Base decoder (ref decoder.py:23-87)."""

    def __init__(self, labels, blank_index=0):
        self.labels = labels
        self.int_to_char = dict([(i, c) for (i, c) in enumerate(labels)])
        self.blank_index = blank_index
        space_index = len(labels)
        if ' ' in labels:
            space_index = labels.index(' ')
        self.space_index = space_index

    def wer(self, s1, s2):
        b = set(s1.split() + s2.split())
        word2char = dict(zip(b, range(len(b))))
        w1 = [chr(word2char[w]) for w in s1.split()]
        w2 = [chr(word2char[w]) for w in s2.split()]
        return _levenshtein(''.join(w1), ''.join(w2))

    def cer(self, s1, s2):
        s1, s2, = s1.replace(' ', ''), s2.replace(' ', '')
        return _levenshtein(s1, s2)

    def decode(self, probs, sizes=None):
        raise NotImplementedError

    def _row_string(self, row) -> str:
        """Label ids (numpy int row) -> string: one UTF-32 table lookup when every label is a
        single character (a per-id Python join cost ~3 ms per 32 x 30 s batch, more than the
        greedy kernel itself)."""
        lut = getattr(self, "_lut32", None)
        if lut is None:
            single = all(len(c) == 1 for c in self.labels)
            lut = np.array([ord(c) for c in self.labels], dtype="<u4") if single else False
            self._lut32 = lut
        if lut is False:
            return ''.join(self.int_to_char[int(c)] for c in row)
        return lut[row].tobytes().decode("utf-32-le")


class BeamCTCDecoder(Decoder):
    """CTC prefix beam search on the GPU (ds2_ctc_beam_decode[_lm]), drop-in for ref
    decoder.py:90-143.

    Same constructor and ``decode(probs, sizes) -> (strings, offsets)`` as the
    reference, whose ctcdecode backend returns every beam: strings[n][p] /
    offsets[n][p] for p < beam_width, best first.  With ``lm_path`` (an ARPA file --
    KenLM's text format; its binary format is not read) the search scores words with
    the n-gram model like ctcdecode's KenLM Scorer (alpha: LM weight, beta: word bonus;
    ds2amd/lm.py builds the device tables once); without an LM ctcdecode ignores
    alpha/beta and so does this.

    Limits: ``beam_width <= 128`` and ``len(labels) <= 64`` (the reference's default beam of
    100 over its Cyrillic label set of 36 is inside them); beyond either the constructor
    raises ``ValueError``.
    """

    def __init__(self, labels, lm_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0,
                 beam_width=100, num_processes=4, blank_index=0):
        super().__init__(labels, blank_index=blank_index)
        self.scorer = None
        if lm_path is not None:
            from .lm import ArpaScorer
            self.scorer = ArpaScorer(lm_path, labels, alpha, beta)
        # the device search is one wave per utterance over u64 char masks: beam_width <= 128
        # and <= 64 labels (three kernel instances: beams <= 32, <= 32 labels, and both above)
        if beam_width > 128 or len(labels) > 64:
            raise ValueError("ds2amd.BeamCTCDecoder: beam_width <= 128 and at most 64 labels "
                             f"(got beam_width={beam_width}, {len(labels)} labels)")
        self.beam_width = int(beam_width)
        self.cutoff_top_n = int(cutoff_top_n)
        self.cutoff_prob = float(cutoff_prob)

    def decode_raw(self, probs, sizes=None):
        """Device tensors (ids [N,P,T], offsets [N,P,T], lens [N,P], scores [N,P])."""
        if self.scorer is not None:
            return ops.ctc_beam_decode_lm_raw(probs, sizes, self.beam_width, self.beam_width,
                                              self.scorer, blank=self.blank_index,
                                              cutoff_top_n=self.cutoff_top_n,
                                              cutoff_prob=self.cutoff_prob)
        return ops.ctc_beam_decode_raw(probs, sizes, self.beam_width, self.beam_width,
                                       blank=self.blank_index, cutoff_top_n=self.cutoff_top_n,
                                       cutoff_prob=self.cutoff_prob)

    def convert_to_strings(self, out, seq_len):
        """[batch][beam][T] label ids (ctcdecode's ``beam_results``) and [batch][beam]
        lengths -> [batch][beam] strings; a beam of length <= 0 is ''.  Ref
        decoder.py:101-113 (tensors, numpy arrays or nested lists)."""
        results = []
        for b, batch in enumerate(out):
            utterances = []
            for p, utt in enumerate(batch):
                size = int(seq_len[b][p])
                row = np.asarray(utt[0:size] if size > 0 else [], dtype=np.int64)
                utterances.append(self._row_string(row) if size > 0 else '')
            results.append(utterances)
        return results

    def convert_tensor(self, offsets, sizes):
        """[batch][beam][T] frame offsets and [batch][beam] lengths -> per beam the first
        ``size`` offsets (an empty int tensor for size <= 0).  Ref decoder.py:115-126."""
        results = []
        for b, batch in enumerate(offsets):
            utterances = []
            for p, utt in enumerate(batch):
                size = int(sizes[b][p])
                if size > 0:
                    utterances.append(utt[0:size])
                else:
                    utterances.append(torch.tensor([], dtype=torch.int))
            results.append(utterances)
        return results

    def decode(self, probs, sizes=None):
        """Ref decoder.py:128-143: (strings, offsets) per utterance and beam, best first;
        the reference's ``convert_to_strings`` / ``convert_tensor`` over the device search's
        (ids, offsets, lens), with one device->host copy and vectorised id->char lookups (a
        per-element tensor loop cost more than the beam search itself on 30 s utterances)."""
        ids, offs, lens, _ = self.decode_raw(probs, sizes)
        ids, offs, lens = ids.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
        strings = self.convert_to_strings(ids, lens)
        offsets = self.convert_tensor(torch.from_numpy(offs), lens)
        return strings, offsets


class StreamingBeamCTCDecoder(BeamCTCDecoder):
    """BeamCTCDecoder over probabilities that arrive in chunks (ds2amd.streaming): the beam,
    its LM state and its prefix trie stay on the device between calls
    (ds2_ctc_beam_stream_feed[_lm]), so a feed costs its own frames only, and after the last
    chunk the result is ``BeamCTCDecoder.decode`` of the concatenated frames, whatever the
    partition.

    ``feed(probs [N, k, C], sizes=None, partial=True) -> (strings, offsets)``: the current
    ``top_paths`` best hypotheses of every stream *in full* (not a delta: the beam may revise
    earlier characters), strings[n][p] / offsets[n][p] best first, offsets in absolute output
    frames; ``sizes`` (int [N]) are this chunk's valid frames per stream, k == 0 is allowed,
    and ``partial=False`` skips the read-out and returns None.  ``finish()`` returns every beam
    in ``decode``'s format, ``text()`` the best string per stream, ``reset()`` starts new
    utterances in the same buffers.  The stream count is fixed by the first ``feed``.

    ``max_frames`` bounds the output frames of one utterance (3000: 60 s of audio); the trie
    is allocated once for it, 36 bytes x max_frames x beam_width per stream (10.8 MB at the
    default beam of 100).  Feeding past it raises ValueError."""

    def __init__(self, labels, lm_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0,
                 beam_width=100, num_processes=4, blank_index=0, max_frames=3000, top_paths=1):
        super().__init__(labels, lm_path=lm_path, alpha=alpha, beta=beta,
                         cutoff_top_n=cutoff_top_n, cutoff_prob=cutoff_prob,
                         beam_width=beam_width, num_processes=num_processes,
                         blank_index=blank_index)
        if self.beam_width < 1 or max_frames < 1 or max_frames * self.beam_width >= 2 ** 31 - 1:
            raise ValueError("ds2amd.StreamingBeamCTCDecoder: beam_width >= 1 and "
                             "1 <= max_frames, max_frames * beam_width < 2^31 - 1 "
                             f"(got beam_width={beam_width}, max_frames={max_frames})")
        if not 1 <= top_paths <= self.beam_width:
            raise ValueError("ds2amd.StreamingBeamCTCDecoder: 1 <= top_paths <= beam_width "
                             f"(got top_paths={top_paths}, beam_width={beam_width})")
        self.max_frames = int(max_frames)
        self.top_paths = int(top_paths)
        self.frames_fed = 0         # the host's count: frames given to feed() so far
        self._state = None
        self._n = None
        self._dev = None

    def _feed_raw(self, probs, sizes, top_paths, readout):
        kw = dict(readout=readout, blank=self.blank_index, cutoff_top_n=self.cutoff_top_n,
                  cutoff_prob=self.cutoff_prob)
        if self.scorer is not None:
            return ops.ctc_beam_stream_feed_lm_raw(self._state, probs, sizes, self.beam_width,
                                                   top_paths, self.scorer, self.max_frames,
                                                   self.frames_fed, **kw)
        return ops.ctc_beam_stream_feed_raw(self._state, probs, sizes, self.beam_width, top_paths,
                                            self.max_frames, self.frames_fed, **kw)

    def _strings(self, raw):
        ids, offs, lens = (x.cpu().numpy() for x in raw[:3])
        return (self.convert_to_strings(ids, lens),
                self.convert_tensor(torch.from_numpy(offs), lens))

    def feed_raw(self, probs, sizes=None, partial=True):
        """``feed`` in device tensors: (ids [N,P,F], offsets [N,P,F], lens [N,P], scores [N,P],
        frames [N]) with P = top_paths and F = the frames fed so far; the first four are None
        with partial=False.  No synchronisation."""
        if probs.dim() != 3 or probs.shape[2] != len(self.labels):
            raise ValueError(f"probs must be [N, k, {len(self.labels)}], got {tuple(probs.shape)}")
        n, k = int(probs.shape[0]), int(probs.shape[1])
        if self._n is not None and n != self._n:
            raise ValueError(f"StreamingBeamCTCDecoder: {self._n} streams since the first feed, "
                             f"got {n}")
        if self.frames_fed + k > self.max_frames:
            raise ValueError(f"StreamingBeamCTCDecoder: {self.frames_fed} + {k} frames exceed "
                             f"max_frames={self.max_frames}")
        if not probs.is_cuda:
            raise RuntimeError("ds2amd StreamingBeamCTCDecoder.feed runs on the GPU (HIP kernel)")
        if n < 1:
            raise ValueError("StreamingBeamCTCDecoder: at least one stream")
        if self._state is None:
            self._n, self._dev = n, probs.device
            self._state = ops.ctc_beam_stream_state(n, self.max_frames, self.beam_width,
                                                    probs.device)
        out = self._feed_raw(probs.detach(), sizes, self.top_paths, partial)
        self.frames_fed += k
        return out

    def feed(self, probs, sizes=None, partial=True):
        raw = self.feed_raw(probs, sizes, partial)
        return self._strings(raw) if partial else None

    def _read(self, top_paths):
        if self._state is None:
            raise RuntimeError("StreamingBeamCTCDecoder: nothing fed yet (the first feed fixes "
                               "the stream count and the device)")
        empty = torch.empty(self._n, 0, len(self.labels), device=self._dev, dtype=torch.float32)
        return self._strings(self._feed_raw(empty, None, top_paths, True))

    def finish(self):
        """(strings, offsets) of every beam, best first: what ``BeamCTCDecoder.decode`` returns
        for the frames fed.  The state is left as it is (more frames may follow)."""
        return self._read(self.beam_width)

    def text(self):
        """Per stream, the best string so far."""
        return [s[0] for s in self._read(1)[0]]

    def reset(self):
        """Every stream back at the start of an utterance, in the same buffers."""
        self.frames_fed = 0
        if self._state is not None:
            ops.ctc_beam_stream_state(self._n, self.max_frames, self.beam_width, self._dev,
                                      out=self._state)


class GreedyDecoder(Decoder):
    def __init__(self, labels, blank_index=0):
        super().__init__(labels, blank_index)

    def convert_to_strings(self, sequences, sizes=None, remove_repetitions=False,
                           return_offsets=False):
        """Host conversion of id sequences (targets) to strings (ref decoder.py:150-163)."""
        strings = []
        offsets = [] if return_offsets else None
        for x in range(len(sequences)):
            seq_len = sizes[x] if sizes is not None else len(sequences[x])
            string, string_offsets = self.process_string(sequences[x], seq_len, remove_repetitions)
            strings.append([string])
            if return_offsets:
                offsets.append([string_offsets])
        if return_offsets:
            return strings, offsets
        return strings

    def process_string(self, sequence, size, remove_repetitions=False):
        seq = [int(v) for v in (sequence.tolist() if torch.is_tensor(sequence) else sequence)]
        size = int(size)
        string = ''
        offsets = []
        blank = self.int_to_char[self.blank_index]
        for i in range(size):
            char = self.int_to_char[seq[i]]
            if char != blank:
                if remove_repetitions and i != 0 and char == self.int_to_char[seq[i - 1]]:
                    pass
                elif char == self.labels[self.space_index] if self.space_index < len(self.labels) else False:
                    string += ' '
                    offsets.append(i)
                else:
                    string = string + char
                    offsets.append(i)
        return string, torch.tensor(offsets, dtype=torch.int)

    def decode_ids(self, probs, sizes=None):
        """Device-side greedy decode; returns (ids, offsets, counts) int32 device tensors."""
        ids, offs, counts, _ = ops.greedy_decode_raw(probs, sizes, blank=self.blank_index)
        return ids, offs, counts

    def decode(self, probs, sizes=None):
        """Returns (strings, offsets) like ref decoder.py:182-197."""
        if not probs.is_cuda:
            raise RuntimeError("ds2amd GreedyDecoder.decode runs on the GPU (HIP kernel)")
        ids, offs, counts = self.decode_ids(probs, sizes)
        ids, offs, counts = ids.cpu().numpy(), offs.cpu().numpy(), counts.cpu().numpy()
        strings, offsets = [], []
        for b in range(ids.shape[0]):
            k = int(counts[b])
            # the space label is ' ' itself, so the label table maps it
            strings.append([self._row_string(ids[b, :k])])
            offsets.append([torch.from_numpy(offs[b, :k].astype(np.int32))])
        return strings, offsets


class StreamingGreedyDecoder(GreedyDecoder):
    """Greedy CTC decoding of probabilities that arrive in chunks (ds2amd.streaming).

    ``feed(probs [N, k, C]) -> (strings_delta, offsets_delta)``: what the k new frames add, per
    stream a one-element list as GreedyDecoder.decode returns; offsets are absolute output-frame
    indices.  The last frame of each call is carried and put in front of the next window of
    ds2_greedy_decode, so a label repeated across a chunk edge collapses as it would inside
    one; the carried frame's own re-emission (offset 0 of the window) is dropped.  ``text()``
    returns everything decoded so far."""

    def __init__(self, labels, blank_index=0):
        super().__init__(labels, blank_index)
        self._carry = None       # [N, 1, C]: the last frame seen
        self._seen = 0           # frames decoded so far
        self._text = None

    def feed(self, probs):
        if not probs.is_cuda:
            raise RuntimeError("ds2amd StreamingGreedyDecoder.feed runs on the GPU (HIP kernel)")
        n, k, _ = probs.shape
        if self._text is None:
            self._text = [''] * n
        if k == 0:
            return [['']] * n, [[torch.zeros(0, dtype=torch.int32)] for _ in range(n)]
        lead = 0 if self._carry is None else 1
        window = probs if lead == 0 else torch.cat([self._carry, probs], 1)
        ids, offs, counts = self.decode_ids(window)
        ids, offs, counts = ids.cpu().numpy(), offs.cpu().numpy(), counts.cpu().numpy()
        strings, offsets = [], []
        for b in range(n):
            c = int(counts[b])
            row, off = ids[b, :c], offs[b, :c]
            if lead:
                keep = off > 0           # offset 0 is the carried frame, emitted by the last call
                row, off = row[keep], off[keep]
            s = self._row_string(row)
            self._text[b] += s
            strings.append([s])
            offsets.append([torch.from_numpy((off - lead + self._seen).astype(np.int32))])
        self._carry = probs[:, -1:].detach().clone()
        self._seen += k
        return strings, offsets

    def text(self):
        """Per stream, the string decoded so far."""
        return list(self._text or [])
