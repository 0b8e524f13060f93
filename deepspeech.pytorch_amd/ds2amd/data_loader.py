"""Feature front-end and batching — drop-in for the hot-path parts of the
reference ``data/data_loader.py`` / ``data/data_loader_aug.py``.

* ``SpectrogramParser.audio_to_stft`` / ``parse_audio`` run the STFT, |.|,
  log1p and 'max_frame' normalisation as one HIP pipeline (ds2_stft_logmag) on
  the GPU instead of librosa in CPU worker processes (ref
  data_loader.py:201-220,276-284; data_loader_aug.py:220-249,297-307).
* ``SpectrogramParser.parse_batch`` takes raw PCM for a whole batch and returns
  the collated, zero-padded [N, 1, 161, T_max] device tensor directly.
* ``_collate_fn``, ``BucketingSampler``, ``DistributedBucketingSampler`` and
  ``AudioDataLoader`` keep the reference's semantics (data_loader_aug.py:523-617).
"""
from __future__ import annotations

import csv
import math
import queue
import random
import re
import threading
from glob import glob
from typing import List, Sequence

import numpy as np
import torch
from torch.utils.data import DataLoader
from torch.utils.data.sampler import Sampler

from . import ops
from .audio_aug import (MAX_RAW_CHANNELS, RESAMPLE, Wave, apply_waves, build_audio_augs,
                        heavy_length, upload_raw)
from .spect_aug import SpectAugmenter

# tempo classes of the reference's legacy sox path (data_loader_aug.py:108-112); only the
# draws they cause are kept (the sox branch itself is dead code there, :690-697)
TEMPOS = {
    0: ('1.0', (1.0, 1.0)),
    1: ('0.9', (0.85, 0.95)),
    2: ('1.1', (1.05, 1.15))
}


def hamming(n: int) -> np.ndarray:
    """scipy.signal.hamming(n) (sym=True): 0.54 - 0.46 cos(2 pi k / (n - 1))."""
    if n == 1:
        return np.ones(1)
    k = np.arange(n)
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * k / (n - 1))


def hann(n: int) -> np.ndarray:
    if n == 1:
        return np.ones(1)
    k = np.arange(n)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / (n - 1))


windows = {'hamming': hamming, 'hann': hann}


def gaussian_taps(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """The correlation weights of scipy.ndimage.gaussian_filter1d (order 0)."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[::-1].copy()


def load_audio_norm(path, channel=-1):
    """scipy wav read + normalise by max |x| (ref data/audio_loader.py:4-27)."""
    from scipy.io import wavfile
    sample_rate, sound = wavfile.read(path)
    abs_max = np.abs(sound).max()
    sound = sound.astype('float32')
    if abs_max > 0:
        sound *= 1 / abs_max
    if len(sound.shape) > 1:
        if sound.shape[1] == 1:
            sound = sound.squeeze()
        elif channel == -1:
            sound = sound.mean(axis=1)
        else:
            sound = sound[:, channel]
    return sound, sample_rate


def load_audio_raw(path, channel=-1):
    """load_audio_norm without the host arithmetic: -> (audio_aug.Wave, sample_rate).  An
    int16 file of at most 8 channels comes back in the raw form (Wave.from_raw: the samples
    are converted on the device, ds2_pcm_decode); any other wav dtype (uint8, int32, float)
    goes through load_audio_norm.  An empty file is an error here as it is there."""
    from scipy.io import wavfile
    sample_rate, sound = wavfile.read(path)
    if sound.shape[0] == 0:
        raise ValueError(f"{path}: wav file without samples")
    if sound.dtype == np.int16 and (sound.ndim == 1 or sound.shape[1] <= MAX_RAW_CHANNELS):
        return Wave.from_raw(sound, channel), sample_rate
    y, sample_rate = load_audio_norm(path, channel=channel)
    return Wave(y), sample_rate


def load_randomly_augmented_audio(path, sample_rate=16000, tempo_range=(0.85, 1.15),
                                  gain_range=(-10, 10), channel=-1, transforms=None,
                                  loader=None):
    """data_loader_aug.py:679-699 (+ augment_audio_with_augs :660-676): the tempo and gain
    draws the reference makes (and no longer uses), the normalised wav, then the
    transforms' records.  -> (audio_aug.Wave, sample_rate).  loader: what reads the file,
    ``loader(path, channel=...)`` -> (samples or Wave, sample rate); load_audio_norm when None."""
    np.random.uniform(low=tempo_range[0], high=tempo_range[1])
    np.random.uniform(low=gain_range[0], high=gain_range[1])
    y, sr = (loader or load_audio_norm)(path, channel=channel)
    wav = y if isinstance(y, Wave) else Wave(y)
    if sr != sample_rate:
        # librosa.resample(y, sr, sample_rate) (data_loader_aug.py:667-668), on the device
        wav.record(RESAMPLE, a=sr, b=sample_rate)
        wav.length = heavy_length(RESAMPLE, sr, sample_rate, 0.0, wav.length)
    if transforms is not None:
        wav = transforms(**{'wav': wav, 'sr': sample_rate})['wav']
    return wav, sample_rate


class SpectrogramParser(object):
    def __init__(self, audio_conf, cache_path=None, normalize=False, augment=False, channel=-1,
                 device=None):
        self.window_stride = audio_conf['window_stride']
        self.window_size = audio_conf['window_size']
        self.sample_rate = audio_conf['sample_rate']
        self.window = windows.get(audio_conf.get('window', 'hamming'), windows['hamming'])
        self.normalize = normalize
        self.augment = augment
        self.channel = channel
        self.cache_path = cache_path
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        self._cache = {}
        # spectrogram augmentations (data_loader_aug.py:241-248), drawn on the host and
        # applied inside the STFT kernel; inactive unless audio_conf enables them
        self.spect_aug = SpectAugmenter(audio_conf)
        # waveform augmentations (data_loader_aug.py:361-418, aug_type 0), drawn on the
        # host and replayed on the device (ds2_wave_aug); None unless noise_prob > 0
        noise_dir = audio_conf.get('noise_dir')
        # glob order unsorted, as the reference's (data_loader_aug.py:363): AddNoise picks a
        # file by index, so the same draws mix in the same file on the same filesystem
        self.augs = build_audio_augs(audio_conf, glob(noise_dir) if noise_dir else ())

    def _consts(self, sample_rate):
        key = sample_rate
        if key not in self._cache:
            n_fft = int(sample_rate * (self.window_size + 1e-8))
            hop = int(sample_rate * (self.window_stride + 1e-8))
            win = torch.tensor(self.window(n_fft), dtype=torch.float64, device=self.device)
            # the gaussian_filter1d of 'max_frame' (sigma 20) / 'frame' (sigma 50)
            sigma = {1: 20, 4: 50}.get(self._mode())
            taps = None if sigma is None else torch.tensor(gaussian_taps(sigma),
                                                            dtype=torch.float32, device=self.device)
            self._cache[key] = (n_fft, hop, win, taps)
        return self._cache[key]

    # normalize_audio (data_loader_aug.py:274-313; --norm, train.py:75) -> ds2_stft_logmag mode
    NORM_MODES = {'none': 0, 'max_frame': 1, 'mean': 2, 'norm': 3, 'frame': 4}

    def _mode(self):
        if not self.normalize:
            return 0
        try:
            return self.NORM_MODES[self.normalize]
        except KeyError:
            raise ValueError(f"normalize={self.normalize!r}: the reference's modes are "
                             f"{sorted(self.NORM_MODES)} (data_loader_aug.py:274-313)") from None

    def parse_batch(self, signals: Sequence, sample_rate=None, draw_order=None):
        """Raw PCM list (numpy arrays, or audio_aug.Wave records of augmented utterances)
        -> (spect [N,1,F,T_max] on device, frames int32 [N]).  draw_order: the rows in the
        order their random draws are made (DeviceBatchLoader: the sampler's order of rows it
        has sorted by length); None = row by row."""
        sr = sample_rate or self.sample_rate
        n_fft, hop, win, taps = self._consts(sr)
        # a zero-length utterance has no spectrogram (np.pad cannot reflect an empty axis in
        # the reference): refused here, before anything is uploaded or launched
        for i, s in enumerate(signals):
            if (s.length if isinstance(s, Wave) else len(s)) < 1:
                raise ValueError(f"parse_batch: utterance {i} has no samples")
        if any(isinstance(s, Wave) and s.records for s in signals):
            pcm_d, lens = apply_waves(signals, self.device)
        else:
            # no transform applied anything: the plain PCM upload, no ds2_wave_aug launch
            lens = [s.n_in if isinstance(s, Wave) else len(s) for s in signals]
            max_s = max(lens)
            # raw int16 utterances: 2 bytes per sample up, decoded on the device
            pcm_d = upload_raw(signals, max_s, self.device)
            if pcm_d is None:
                signals = [s.samples if isinstance(s, Wave) else s for s in signals]
                pcm = np.zeros((len(signals), max_s), dtype=np.float32)
                for i, s in enumerate(signals):
                    pcm[i, :len(s)] = s
                pcm_d = torch.from_numpy(pcm).to(self.device)
        ns_d = torch.tensor(lens, dtype=torch.int32).to(self.device)
        frames = [ops.stft_frames(n, n_fft, hop) for n in lens]
        # the per-utterance draws (mask bands, offset) go row by row, or through the rows in
        # draw_order: draw k belongs to row draw_order[k]
        pos = None
        if draw_order is not None:
            if sorted(draw_order) != list(range(len(signals))):
                raise ValueError("parse_batch: draw_order must be a permutation of the rows")
            pos = torch.empty(len(signals), dtype=torch.long)
            pos[torch.tensor(list(draw_order), dtype=torch.long)] = torch.arange(len(signals))
        masks = self.spect_aug.masks(ops.SPECT_ROWS, frames if pos is None else
                                     [frames[r] for r in draw_order], self.device)
        if masks is not None and pos is not None:
            masks = masks[pos.to(self.device)].contiguous()
        out = ops.stft_logmag(pcm_d, ns_d, n_fft, hop, win, self._mode(), taps, max(frames),
                              masks=masks)
        if self.augment and self.normalize == 'max_frame':
            # one U(-0.5, 0.5) offset per utterance on its valid frames (data_loader_aug.py:213-214)
            off = torch.rand(len(signals)) - 0.5
            off = (off if pos is None else off[pos]).to(self.device)
            mask = (torch.arange(max(frames), device=self.device)[None, :] <
                    torch.tensor(frames, device=self.device)[:, None]).float()
            out = out + off[:, None, None] * mask[:, None, :]
        return out.unsqueeze(1), torch.tensor(frames, dtype=torch.int32)

    def audio_to_stft(self, y, sample_rate):
        """Single utterance (PCM or audio_aug.Wave) -> normalised spectrogram [F, T]
        (device tensor)."""
        if not isinstance(y, Wave):
            y = np.asarray(y, dtype=np.float32)
        spect, _ = self.parse_batch([y], sample_rate)
        return spect[0, 0]

    def parse_audio(self, audio_path):
        """data_loader_aug.py:163-215 with the reference's draws: tempo class (augment
        only), the two unused sox draws, then the waveform augs (self.augs)."""
        tempo_id = random.randrange(3) if self.augment else 0
        y, sr = load_randomly_augmented_audio(audio_path, self.sample_rate, channel=self.channel,
                                              tempo_range=TEMPOS[tempo_id][1],
                                              transforms=self.augs)
        return self.audio_to_stft(y, sr)

    def parse_audio_for_transcription(self, audio_path):
        return self.parse_audio(audio_path)


def _collate_fn(batch):
    """Sort by length desc, zero-pad to [N,1,F,T_max] (ref data_loader_aug.py:523-548)."""
    batch = sorted(batch, key=lambda sample: sample[0].size(1), reverse=True)
    longest_sample = max(batch, key=lambda p: p[0].size(1))[0]
    freq_size = longest_sample.size(0)
    minibatch_size = len(batch)
    max_seqlength = longest_sample.size(1)
    inputs = torch.zeros(minibatch_size, 1, freq_size, max_seqlength)
    input_percentages = torch.FloatTensor(minibatch_size)
    target_sizes = torch.IntTensor(minibatch_size)
    targets = []
    filenames = []
    for x in range(minibatch_size):
        tensor, target = batch[x][0], batch[x][1]
        filenames.append(batch[x][2] if len(batch[x]) > 2 else None)
        seq_length = tensor.size(1)
        inputs[x][0].narrow(1, 0, seq_length).copy_(tensor)
        input_percentages[x] = seq_length / float(max_seqlength)
        target_sizes[x] = len(target)
        targets.extend(target)
    targets = torch.IntTensor(targets)
    return inputs, targets, filenames, input_percentages, target_sizes


class AudioDataLoader(DataLoader):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.collate_fn = _collate_fn


class BucketingSampler(Sampler):
    def __init__(self, data_source, batch_size=1):
        self.data_source = data_source
        ids = list(range(0, len(data_source)))
        self.bins = [ids[i:i + batch_size] for i in range(0, len(ids), batch_size)]

    def __iter__(self):
        for ids in self.bins:
            np.random.shuffle(ids)
            yield ids

    def __len__(self):
        return len(self.bins)

    def shuffle(self, epoch):
        np.random.shuffle(self.bins)


class DistributedBucketingSampler(Sampler):
    """Rank r takes bins[r::world], padded to an even split (ref data_loader_aug.py:582-617)."""

    def __init__(self, data_source, batch_size=1, num_replicas=None, rank=None):
        if num_replicas is None or rank is None:
            import torch.distributed as dist
            num_replicas = dist.get_world_size() if num_replicas is None else num_replicas
            rank = dist.get_rank() if rank is None else rank
        self.data_source = data_source
        self.ids = list(range(0, len(data_source)))
        self.batch_size = batch_size
        self.bins = [self.ids[i:i + batch_size] for i in range(0, len(self.ids), batch_size)]
        self.num_replicas = num_replicas
        self.rank = rank
        self.num_samples = int(math.ceil(len(self.bins) * 1.0 / self.num_replicas))
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        bins = self.bins + self.bins[:(self.total_size - len(self.bins))]
        assert len(bins) == self.total_size
        return iter(bins[self.rank::self.num_replicas])

    def __len__(self):
        return self.num_samples

    def shuffle(self, epoch):
        g = torch.Generator()
        g.manual_seed(epoch)
        bin_ids = list(torch.randperm(len(self.bins), generator=g))
        self.bins = [self.bins[i] for i in bin_ids]


def _roman_numerals():
    """The Roman numerals the reference's transcripts may hold, 2 to 40 ('XXXX' for 40, as its
    table writes it; data/labels.py:5-10)."""
    tens = ['', 'X', 'XX', 'XXX']
    units = ['', 'I', 'II', 'III', 'IV', 'V', 'VI', 'VII', 'VIII', 'IX']
    table = {tens[v // 10] + units[v % 10]: v for v in range(2, 40)}
    table['XXXX'] = 40
    return table


ROMAN = _roman_numerals()


class Labels(object):
    """Transcript text <-> label ids (ref data/labels.py:13-61).

    ``parse`` keeps the reference's steps: the '2' that marks a doubled letter in a
    transcript is dropped, '*' and '+' become spaces and '%' the word 'процент', 'ё' becomes
    'е', the text is cut into words, every character outside the label set is dropped, the
    words are joined by single spaces and upper-cased, and a code equal to the one before it
    is written as the code of '2'.  Nothing left gives '*'.  A text that starts with
    '!clean:' is mapped character by character with none of this.  A character the label set
    lacks ('*' or '2' with labels that have neither) is a KeyError.

    The reference spells numbers out through a ``num2word`` module that it does not contain,
    so what a digit word or a Roman numeral should become is unknown: both raise
    NotImplementedError."""

    WORD = re.compile(r'-?\d+|-?\d+-\w+|\w+')

    def __init__(self, labels):
        self.labels = labels
        self.labels_map = {c: i for i, c in enumerate(labels)}

    def _number(self, word):
        raise NotImplementedError(
            f"Labels.parse: {word!r} needs the number expansion of the reference's num2word "
            "module, which the reference does not contain")

    def find_words(self, text, clean=True):
        text = re.sub(r'([^\W\d]+)2', r'\1', text)
        for old, new in (('*', ' '), ('+', ' '), ('%', 'процент*'), ('ё', 'е'), ('Ё', 'Е')):
            text = text.replace(old, new)
        words = []
        for w in self.WORD.findall(text):
            if w in ROMAN or w.isdigit():
                self._number(w)
            if '-' in w:
                head, rest = w.split('-', 1)
                if head.isdigit() and not rest.isdigit():
                    self._number(w)
            if clean:
                w = ''.join(c for c in w if c.upper() in self.labels_map).strip()
            if w:
                words.append(w)
        return words

    def parse(self, text):
        if text.startswith('!clean:'):
            return [self.labels_map[c] for c in text.replace('!clean:', '', 1).strip()]
        chars = ' '.join(self.find_words(text)).upper().strip() or '*'
        codes = []
        for c in chars:
            code = self.labels_map[c]
            if codes and codes[-1] == code:
                code = self.labels_map['2']
            codes.append(code)
        return codes

    def render_transcript(self, codes):
        return ''.join(self.labels[i] for i in codes)


class SpectrogramDataset(SpectrogramParser):
    """Manifest -> (spectrogram, target ids, wav path): the reference's SpectrogramDataset
    (data_loader_aug.py:322-460,505-520) on the device front-end.

    The manifest is CSV, one utterance per row: ``wav path,transcript path[,duration]``.
    ``__getitem__`` is the reference's, one utterance per call (and so one set of launches
    per utterance): it is there for AudioDataLoader; a training loop reads whole bins through
    DeviceBatchLoader, which uses ``load_item``.  The curriculum sampling of
    data/curriculum.py is not built; ``set_curriculum_epoch`` reshuffles only."""

    def __init__(self, audio_conf, manifest_filepath, cache_path, labels, normalize=False,
                 augment=False, max_items=None, device=None):
        with open(manifest_filepath, newline='') as f:
            ids = [(row[0], row[1], row[2] if len(row) > 2 else 0) for row in csv.reader(f)]
        if max_items:
            ids = ids[:max_items]
        self.all_ids = ids
        self.ids = ids
        self.size = len(ids)
        self.labels = Labels(labels)
        self._transcripts = {}
        super().__init__(audio_conf, cache_path, normalize, augment, device=device)

    def __len__(self):
        return self.size

    def parse_transcript(self, transcript_path):
        """Target ids of a transcript file, parsed once per path ('' parses the empty text)."""
        if transcript_path not in self._transcripts:
            if not transcript_path:
                ts = self.labels.parse('')
            else:
                with open(transcript_path, 'r', encoding='utf8') as f:
                    ts = self.labels.parse(f.read())
            self._transcripts[transcript_path] = ts
        return self._transcripts[transcript_path]

    def get_reference_transcript(self, txt):
        return self.labels.render_transcript(self.parse_transcript(txt))

    def set_curriculum_epoch(self, epoch):
        """data_loader_aug.py:480-483: all ids, reshuffled under np.random.seed(epoch)."""
        self.ids = list(self.all_ids)
        np.random.seed(epoch)
        np.random.shuffle(self.ids)
        self.size = len(self.ids)

    def load_item(self, index, loaded=None):
        """-> (audio_aug.Wave, sample_rate, target ids, wav path), no GPU call.  The host
        draws of parse_audio in its order (tempo class when augmenting, the two unused sox
        draws, the waveform transforms); the samples stay int16 (load_audio_raw).  loaded:
        the (Wave, sample rate) of this file when it was read ahead."""
        audio_path, transcript_path = self.ids[index][0], self.ids[index][1]
        tempo_id = random.randrange(3) if self.augment else 0
        loader = load_audio_raw if loaded is None else (lambda path, channel=-1: loaded)
        wav, sr = load_randomly_augmented_audio(audio_path, self.sample_rate,
                                                channel=self.channel,
                                                tempo_range=TEMPOS[tempo_id][1],
                                                transforms=self.augs, loader=loader)
        return wav, sr, self.parse_transcript(transcript_path), audio_path

    def __getitem__(self, index):
        wav, sr, reference, audio_path = self.load_item(index)
        return self.audio_to_stft(wav, sr), reference, audio_path


class DeviceBatchLoader(object):
    """Bins of a BucketingSampler / DistributedBucketingSampler -> the collate tuple of
    ``_collate_fn`` with the inputs built on the device: (inputs [N,1,161,T_max] device,
    targets IntTensor flat, filenames, input_percentages FloatTensor, target_sizes
    IntTensor), what Trainer.train_batch takes.

    The utterances of a bin are ordered by frame count, longest first (ties keep the
    sampler's order, as sorted(..., reverse=True) does), before parse_batch, so its output
    is the collated tensor.  With ``prefetch > 0`` one thread reads the wav and transcript
    files of the next ``prefetch`` bins ahead; it draws no random number and makes no GPU
    call.  Every draw is made by the consuming thread: the sampler's (when the epoch starts:
    ``iter(loader)`` walks the sampler once), then per bin the utterances' host draws in the
    sampler's order (load_item), then the spectrogram masks and the 'max_frame' offsets, also
    in the sampler's order (parse_batch's draw_order).  The batches of a seeded run do not
    depend on ``prefetch``."""

    def __init__(self, dataset, batch_sampler, prefetch=2):
        self.dataset = dataset
        self.batch_sampler = batch_sampler
        self.prefetch = int(prefetch)
        self._thread = None
        self._stop = None
        self._queue = None
        self._bins = iter(())

    def __len__(self):
        return len(self.batch_sampler)

    # ---- the reading thread -----------------------------------------------------------
    def _read_bin(self, ids):
        """[(Wave, sample rate)] of a bin; an error is re-raised with the file's path."""
        out = []
        for i in ids:
            audio_path, transcript_path = self.dataset.ids[i][0], self.dataset.ids[i][1]
            try:
                out.append(load_audio_raw(audio_path, self.dataset.channel))
                self.dataset.parse_transcript(transcript_path)
            except Exception as e:
                raise RuntimeError(f"DeviceBatchLoader: {audio_path}: "
                                   f"{type(e).__name__}: {e}") from e
        return out

    def _reader(self, bins, stop, out):
        for ids in bins:
            try:
                item = (ids, self._read_bin(ids), None)
            except Exception as e:      # handed to the consumer
                item = (ids, None, e)
            while not stop.is_set():
                try:
                    out.put(item, timeout=0.05)
                    break
                except queue.Full:
                    pass
            if stop.is_set() or item[2] is not None:
                return

    def close(self):
        """Stop and join the reading thread (also done at exhaustion and on an error)."""
        t, self._thread = self._thread, None
        if t is not None:
            self._stop.set()
            t.join()
        self._bins = iter(())

    def __iter__(self):
        self.close()
        bins = [list(ids) for ids in self.batch_sampler]     # the sampler's draws, now
        if self.prefetch > 0 and bins:
            self._stop = threading.Event()
            self._queue = queue.Queue(maxsize=self.prefetch)
            self._thread = threading.Thread(target=self._reader, name="ds2-wav-reader",
                                            args=(bins, self._stop, self._queue), daemon=True)
            self._thread.start()
        self._bins = iter(bins)
        return self

    def __next__(self):
        try:
            ids = next(self._bins)
        except StopIteration:
            self.close()
            raise
        try:
            if self._thread is not None:
                got, loaded, err = self._queue.get()
                if err is not None:
                    raise err
                assert got == ids
            else:
                loaded = self._read_bin(ids)
            return self.collate([self.dataset.load_item(i, loaded=l)
                                 for i, l in zip(ids, loaded)])
        except BaseException:
            self.close()
            raise

    def collate(self, items):
        """[(Wave, sample rate, target ids, path)] in the sampler's order -> the batch."""
        ds = self.dataset
        rates = {sr for _, sr, _, _ in items}
        if len(rates) != 1:
            raise ValueError(f"DeviceBatchLoader: one sample rate per batch, got {sorted(rates)}")
        sr = rates.pop()
        n_fft = int(sr * (ds.window_size + 1e-8))
        hop = int(sr * (ds.window_stride + 1e-8))
        rows = sorted(range(len(items)),
                      key=lambda p: ops.stft_frames(items[p][0].length, n_fft, hop),
                      reverse=True)                     # row x holds the sampler's item rows[x]
        draw_order = [rows.index(p) for p in range(len(items))]
        items = [items[p] for p in rows]
        inputs, frames = ds.parse_batch([it[0] for it in items], sr, draw_order=draw_order)
        t_max = int(inputs.size(3))
        n = len(items)
        input_percentages = torch.FloatTensor(n)
        target_sizes = torch.IntTensor(n)
        targets = []
        for x, (_, _, target, _) in enumerate(items):
            input_percentages[x] = int(frames[x]) / float(t_max)
            target_sizes[x] = len(target)
            targets.extend(target)
        return (inputs, torch.IntTensor(targets), [it[3] for it in items], input_percentages,
                target_sizes)
