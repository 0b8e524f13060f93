"""CPU: the host side of training from a manifest -- Labels, the SpectrogramDataset manifest
and transcript handling, the raw (int16) Wave and its lazy float form, load_audio_raw, and
DeviceBatchLoader's ordering, collate bookkeeping and reading thread with parse_batch
replaced by a CPU stub.  No GPU call is made."""
import os
import threading

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from ds2amd import data_loader as dl
from ds2amd.audio_aug import Wave
from ds2amd.data_loader import (BucketingSampler, DeviceBatchLoader, Labels, SpectrogramDataset,
                                load_audio_norm, load_audio_raw)

EN = "_'ABCDEFGHIJKLMNOPQRSTUVWXYZ2 "
RU = "_АБВГДЕЖЗИЙКЛМНОПРСТУФХЦЧШЩЪЫЬЭЮЯ2* "
CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')


def _ids(labels, s):
    return [labels.index(c) for c in s]


# ---------------------------------------------------------------------------------- Labels
def test_labels_parse_known_answers():
    en = Labels(EN)
    assert en.parse("the cat") == _ids(EN, "THE CAT")
    # a doubled letter: the second code is that of '2'; punctuation and digits-free junk drop
    assert en.parse("Hello, world!") == _ids(EN, "HEL2O WORLD")
    assert en.parse("aaa") == _ids(EN, "A2A")
    # a '2' written after letters in the text is dropped before the split
    assert en.parse("hel2o") == _ids(EN, "HELO")
    # characters outside the map vanish, also from inside a word; '*' and '+' split words
    assert en.parse("naïve café a*b+c") == _ids(EN, "NAVE CAF A B C")
    # '!clean:' maps the stripped rest as it stands: no upper-casing, no doubling rule
    assert en.parse("!clean: HELLO \n") == _ids(EN, "HELLO")
    with pytest.raises(KeyError):
        en.parse("!clean:hello")
    # nothing left -> '*', which the English labels do not have
    with pytest.raises(KeyError):
        en.parse("")
    with pytest.raises(KeyError):
        en.parse("?!")


def test_labels_cyrillic_and_star():
    ru = Labels(RU)
    assert ru.parse("ёлка Ёж") == _ids(RU, "ЕЛКА ЕЖ")
    assert ru.parse("") == _ids(RU, "*")
    assert ru.parse("пять %") == _ids(RU, "ПЯТЬ ПРОЦЕНТ")
    assert ru.parse("!clean:ДА*") == _ids(RU, "ДА*")


@pytest.mark.parametrize("text", ["room 101", "в 1999 году", "глава XIV", "XXXX", "5"])
def test_labels_numbers_not_guessed(text):
    with pytest.raises(NotImplementedError, match="num2word"):
        Labels(RU).parse(text)


def test_labels_render_round_trip():
    en = Labels(EN)
    codes = en.parse("a little bookkeeper")
    assert en.render_transcript(codes) == "A LIT2LE BO2K2E2PER"
    assert en.parse("!clean:" + en.render_transcript(codes)) == codes


# -------------------------------------------------------------------------------- manifest
def _wav(path, data, sr=16000):
    wavfile.write(path, sr, data)
    return path


def _dataset(tmp_path, frames, texts=None, **kw):
    rng = np.random.default_rng(0)
    rows = []
    for i, n in enumerate(frames):
        w = _wav(os.path.join(str(tmp_path), f"u{i}.wav"),
                 rng.integers(-3000, 3000, size=n).astype(np.int16))
        t = os.path.join(str(tmp_path), f"u{i}.txt")
        with open(t, "w", encoding="utf8") as f:
            f.write((texts or {}).get(i, f"utterance {'abcdefghij'[i]}"))
        rows.append((w, t))
    man = os.path.join(str(tmp_path), "manifest.csv")
    with open(man, "w", newline="") as f:
        for w, t in rows:
            f.write(f"{w},{t}\n")
    return SpectrogramDataset(CONF, man, None, EN, device="cpu", **kw), rows


def test_manifest_columns_max_items_and_quoted_comma(tmp_path):
    man = os.path.join(str(tmp_path), "m.csv")
    with open(man, "w", newline="") as f:
        f.write('a.wav,a.txt\n"dir, with comma/b.wav",b.txt,3.5\nc.wav,,1.0\n')
    ds = SpectrogramDataset(CONF, man, None, EN, device="cpu")
    assert ds.ids == [("a.wav", "a.txt", 0), ("dir, with comma/b.wav", "b.txt", "3.5"),
                      ("c.wav", "", "1.0")]
    assert len(ds) == 3 and ds.all_ids == ds.ids
    ds = SpectrogramDataset(CONF, man, None, EN, max_items=2, device="cpu")
    assert len(ds) == 2 and ds.ids[-1][0] == "dir, with comma/b.wav"
    assert isinstance(ds, dl.SpectrogramParser)


def test_parse_transcript_is_cached_per_path(tmp_path):
    ds, rows = _dataset(tmp_path, [100, 200])
    t = rows[0][1]
    first = ds.parse_transcript(t)
    assert first == _ids(EN, "UT2ERANCE A")
    os.remove(t)
    assert ds.parse_transcript(t) is first          # not read again
    assert ds.get_reference_transcript(t) == "UT2ERANCE A"
    with pytest.raises(KeyError):                   # '' -> '*', not an English label
        ds.parse_transcript('')
    with pytest.raises(FileNotFoundError):
        ds.parse_transcript(t + ".missing")


def test_set_curriculum_epoch_is_a_seeded_shuffle(tmp_path):
    ds, _ = _dataset(tmp_path, [100, 200, 300, 400, 500])
    for e in (0, 3, 3):
        ds.set_curriculum_epoch(e)
        ref = list(ds.all_ids)
        np.random.seed(e)
        np.random.shuffle(ref)
        assert ds.ids == ref and len(ds) == 5
    assert ds.ids != ds.all_ids


# -------------------------------------------------------------------------------- raw Wave
def _edge_files(tmp_path):
    rng = np.random.default_rng(5)
    r = lambda *s: rng.integers(-32768, 32768, size=s).astype(np.int16)     # noqa: E731
    last = rng.integers(-30000, 30000, size=(4097, 2)).astype(np.int16)
    last[-1, 1] = 32001
    neg = rng.integers(-30000, 30000, size=300).astype(np.int16)
    neg[17] = -32767
    pos = neg.copy()
    pos[17] = 32767
    data = dict(one=r(1), odd=r(257), col=r(65, 1), st=r(255, 2), tri=r(64, 3), oct=r(63, 8),
                zero=np.zeros(65, np.int16), wrap=np.array([-32768, 100, -7], np.int16),
                allmin=np.full(63, -32768, np.int16), neg=neg, pos=pos, last=last)
    return {k: _wav(os.path.join(str(tmp_path), k + ".wav"), v) for k, v in data.items()}, data


def test_raw_wave_samples_equal_load_audio_norm(tmp_path):
    files, data = _edge_files(tmp_path)
    for name, path in files.items():
        ch = 1 if data[name].ndim == 1 else data[name].shape[1]
        for sel in {-1, 0, ch - 1}:
            w, sr = load_audio_raw(path, sel)
            assert sr == 16000 and w.raw is not None and w._samples is None, name
            assert w.length == w.n_in == data[name].shape[0] and w.shape == (w.length,)
            ref, _ = load_audio_norm(path, sel)
            got = w.samples
            assert got.dtype == np.float32 and got.ndim == 1
            assert got.tobytes() == np.ascontiguousarray(ref.reshape(-1)).tobytes(), (name, sel)
            assert w.samples is got                  # computed once
    assert Wave.from_raw(data["wrap"]).samples.tolist() == [np.float32(-327.68), 1.0,
                                                            np.float32(-0.07)]
    # a float Wave is what it was
    w = Wave(np.arange(5, dtype=np.float64))
    assert w.raw is None and w.samples.dtype == np.float32 and w.length == w.n_in == 5


def test_from_raw_rejects_what_the_kernel_cannot_take():
    with pytest.raises(ValueError):
        Wave.from_raw(np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        Wave.from_raw(np.zeros((4, 9), np.int16))
    with pytest.raises(IndexError):
        Wave.from_raw(np.zeros((4, 2), np.int16), 2)
    assert Wave.from_raw(np.zeros((4, 1), np.int16), 5).channel == -1    # mono ignores it


def test_load_audio_raw_fallback_and_empty(tmp_path):
    rng = np.random.default_rng(2)
    f32 = _wav(os.path.join(str(tmp_path), "f.wav"), rng.standard_normal(300).astype(np.float32))
    w, sr = load_audio_raw(f32)
    assert w.raw is None and sr == 16000
    assert np.array_equal(w.samples, load_audio_norm(f32)[0])
    u8 = _wav(os.path.join(str(tmp_path), "u.wav"), rng.integers(0, 255, 300).astype(np.uint8))
    assert load_audio_raw(u8)[0].raw is None
    empty = _wav(os.path.join(str(tmp_path), "e.wav"), np.zeros(0, np.int16))
    with pytest.raises(ValueError, match="e.wav"):
        load_audio_raw(empty)
    with pytest.raises(ValueError):
        load_audio_norm(empty)


# ---------------------------------------------------------------------------------- loader
def _stub_parse_batch(ds, calls):
    def parse_batch(signals, sample_rate=None, draw_order=None):
        frames = [1 + s.length // 160 for s in signals]
        calls.append([s.length for s in signals])
        ds.draw_orders = getattr(ds, "draw_orders", []) + [draw_order]
        x = torch.zeros(len(signals), 1, 161, max(frames))
        for i, f in enumerate(frames):
            x[i, 0, :, :f] = float(signals[i].length)
        return x, torch.tensor(frames, dtype=torch.int32)
    ds.parse_batch = parse_batch


def _reader_threads():
    return [t for t in threading.enumerate() if t.name == "ds2-wav-reader"]


@pytest.mark.parametrize("prefetch", [0, 2])
def test_loader_sort_and_collate_bookkeeping(tmp_path, prefetch):
    # frames (1 + n // 160): 4, 11, 7, 11, 2 -> order 1, 3 (tie: sampler order), 2, 0, 4
    lens = [480, 1600, 1000, 1700, 200]
    ds, rows = _dataset(tmp_path, lens)
    calls = []
    _stub_parse_batch(ds, calls)
    sampler = BucketingSampler(ds, batch_size=5)
    sampler.bins = [[4, 3, 0, 1, 2]]
    np.random.seed(1)
    order = list(sampler.bins[0])
    np.random.shuffle(order)                        # what iterating the sampler will draw
    np.random.seed(1)
    loader = DeviceBatchLoader(ds, sampler, prefetch=prefetch)
    assert len(loader) == 1
    batches = list(loader)
    assert len(batches) == 1 and not _reader_threads()
    inputs, targets, names, pct, sizes = batches[0]
    fr = {i: 1 + n // 160 for i, n in enumerate(lens)}
    want = sorted(order, key=lambda i: fr[i], reverse=True)
    assert [fr[i] for i in want] == [11, 11, 7, 4, 2]
    assert names == [rows[i][0] for i in want]
    assert calls == [[lens[i] for i in want]]
    # the batch's draws stay in the sampler's order: draw k is for the row of its item k
    assert ds.draw_orders == [[want.index(i) for i in order]]
    assert inputs.shape == (5, 1, 161, 11)
    assert pct.dtype == torch.float32 and sizes.dtype == torch.int32
    assert targets.dtype == torch.int32
    ref_pct = torch.FloatTensor(5)
    for x, i in enumerate(want):
        ref_pct[x] = fr[i] / float(11)
    assert torch.equal(pct, ref_pct)
    tg = [ds.parse_transcript(rows[i][1]) for i in want]
    assert sizes.tolist() == [len(t) for t in tg]
    assert targets.tolist() == [c for t in tg for c in t]
    # the same tuple _collate_fn builds from per-item spectrograms
    items = [(inputs[x, 0, :, :fr[i]].clone(), tg[x], rows[i][0]) for x, i in enumerate(want)]
    ref = dl._collate_fn(items)
    assert torch.equal(ref[0], inputs) and torch.equal(ref[1], targets) and ref[2] == names
    assert torch.equal(ref[3], pct) and torch.equal(ref[4], sizes)


def test_prefetch_thread_lifecycle_and_errors(tmp_path):
    ds, rows = _dataset(tmp_path, [300, 400, 500, 600, 700, 800])
    _stub_parse_batch(ds, [])
    sampler = BucketingSampler(ds, batch_size=2)
    loader = DeviceBatchLoader(ds, sampler, prefetch=2)
    assert not _reader_threads()
    it = iter(loader)
    assert len(_reader_threads()) == 1
    next(it)
    loader.close()                                   # abandoned mid-epoch
    assert not _reader_threads()
    with pytest.raises(StopIteration):
        next(it)
    assert len(list(loader)) == 3 and not _reader_threads()      # a new epoch, to the end
    # the thread draws nothing: the random streams after an epoch do not depend on prefetch
    states = []
    for prefetch in (0, 2):
        sampler.bins = [[0, 1], [2, 3], [4, 5]]
        np.random.seed(4)
        names =[b[2] for b in DeviceBatchLoader(ds, sampler, prefetch=prefetch)]
        states.append((names, np.random.get_state()[1].tolist()))
    assert states[0] == states[1]
    # a missing file: raised in the consumer with its path, thread joined
    os.remove(rows[3][0])
    for prefetch in (0, 2):
        loader = DeviceBatchLoader(ds, sampler, prefetch=prefetch)
        with pytest.raises(RuntimeError, match="u3.wav"):
            list(loader)
        assert not _reader_threads()
