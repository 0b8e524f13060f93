"""Inference entry points on the HIP path (ref transcribe.py:33-71).

`transcribe` keeps the reference's single-utterance signature; `transcribe_batch`
is the batched variant SURVEY §8f#1 asks for (cfg5: many long utterances per
forward): raw PCM (or wav paths) -> device STFT -> DeepSpeech.forward in eval mode
-> Greedy/Beam decoder, with one host copy of the decoded ids at the end.

`align_batch` times a known transcript instead of decoding: the same front end and
forward, then the CTC forced alignment of the transcript's label ids on the logits
(`ctc.forced_align`, ds2_ctc_align), returned as character and word frame spans.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Union

import numpy as np
import torch

from .ctc import forced_align
from .data_loader import Labels, SpectrogramParser, load_audio_norm
from .decoder import Decoder


def transcribe(audio_path, parser: SpectrogramParser, model, decoder, device=None):
    """ref transcribe.py:63-71: one wav file -> (decoded_output, decoded_offsets)."""
    return transcribe_batch([audio_path], parser, model, decoder)


def transcribe_batch(audio: Sequence[Union[str, np.ndarray]], parser: SpectrogramParser, model,
                     decoder, sample_rate=None):
    """Batched transcription: wav paths or float32 PCM arrays (normalised to max |x| = 1,
    like data/audio_loader.py) -> (decoded_output[N][paths], decoded_offsets[N][paths])."""
    signals: List[np.ndarray] = []
    sr = sample_rate
    for a in audio:
        if isinstance(a, (str, os.PathLike)):
            y, sr_a = load_audio_norm(a, channel=parser.channel)
            sr = sr or sr_a
            signals.append(y)
        else:
            signals.append(np.asarray(a, dtype=np.float32))
    was_training = model.training
    model.eval()
    with torch.no_grad():
        spect, frames = parser.parse_batch(signals, sr)
        _, probs, out_lens = model(spect, frames)
        decoded_output, decoded_offsets = decoder.decode(probs, out_lens)
    model.train(was_training)
    return decoded_output, decoded_offsets


def frame_to_seconds(frame, parser: SpectrogramParser):
    """Start time of an output frame of the model: the convolutions halve the spectrogram's
    frame rate, so one output frame is 2 * window_stride seconds."""
    return frame * 2.0 * parser.window_stride


def transcript_ids(text, labels):
    """Label ids of a transcript.  `labels` is a data_loader.Labels (its `parse`, the
    training pipeline's mapping) or the label string / list a Decoder takes, which maps
    character by character (the inverse of Decoder.int_to_char)."""
    if isinstance(labels, Labels):
        return labels.parse(text)
    table = {c: i for i, c in enumerate(labels)}
    try:
        return [table[c] for c in text]
    except KeyError as e:
        raise ValueError(f"align_batch: character {e.args[0]!r} is not in the label set") from None


def align_batch(audio: Sequence[Union[str, np.ndarray]], transcripts: Sequence[str],
                parser: SpectrogramParser, model, labels, sample_rate=None, blank_index=0):
    """Forced alignment of known transcripts: wav paths or float32 PCM arrays plus one string
    each -> per utterance {'chars': [(char, start_frame, end_frame)], 'words': [(word,
    start_frame, end_frame)] (split at the space label), 'score': log-probability of the
    alignment}, or None where the transcript does not fit the utterance's frames.  Frames are
    the model's output frames, end exclusive; `frame_to_seconds` converts them."""
    first = next(model.parameters(), None)
    if first is None or not first.is_cuda:
        raise RuntimeError("ds2amd align_batch runs on the GPU (HIP kernels); move the model "
                           "there first")
    if len(audio) != len(transcripts):
        raise ValueError("align_batch: one transcript per utterance")
    label_set = labels.labels if isinstance(labels, Labels) else labels
    space = Decoder(label_set, blank_index=blank_index).space_index
    ids = [transcript_ids(t, labels) for t in transcripts]
    signals: List[np.ndarray] = []
    sr = sample_rate
    for a in audio:
        if isinstance(a, (str, os.PathLike)):
            y, sr_a = load_audio_norm(a, channel=parser.channel)
            sr = sr or sr_a
            signals.append(y)
        else:
            signals.append(np.asarray(a, dtype=np.float32))
    was_training = model.training
    model.eval()
    with torch.no_grad():
        spect, frames = parser.parse_batch(signals, sr)
        logits, _, out_lens = model(spect, frames)
        res = forced_align(logits.transpose(0, 1).contiguous(),
                           torch.tensor([i for u in ids for i in u], dtype=torch.int32),
                           out_lens, torch.tensor([len(u) for u in ids], dtype=torch.int32),
                           blank=blank_index)
    model.train(was_training)
    scores = res.scores.cpu().tolist()
    out = []
    for u, spans, score in zip(ids, res.spans, scores):
        if score == float("-inf"):
            out.append(None)
            continue
        spans = spans.cpu().tolist()
        chars = [(label_set[i], s0, s1) for i, (s0, s1) in zip(u, spans)]
        words, cur = [], []
        for i, (ch, s0, s1) in zip(u, chars):
            if i == space:
                if cur:
                    words.append((''.join(c for c, _, _ in cur), cur[0][1], cur[-1][2]))
                cur = []
            else:
                cur.append((ch, s0, s1))
        if cur:
            words.append((''.join(c for c, _, _ in cur), cur[0][1], cur[-1][2]))
        out.append({'chars': chars, 'words': words, 'score': score})
    return out


def decode_results(decoded_output, decoded_offsets, top_paths=1, offsets=False, meta=None):
    """ref transcribe.py:33-60 (the JSON body the reference CLI prints)."""
    results = {"output": []}
    if meta is not None:
        results["_meta"] = meta
    for b in range(len(decoded_output)):
        for pi in range(min(top_paths, len(decoded_output[b]))):
            result = {'transcription': decoded_output[b][pi]}
            if offsets:
                result['offsets'] = decoded_offsets[b][pi].tolist()
            results['output'].append(result)
    return results
