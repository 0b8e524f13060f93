"""GPU: training from a manifest -- SpectrogramDataset + DeviceBatchLoader against the
reference's collate over oracle spectrograms, against the dataset's own __getitem__,
prefetch invariance under augmentation, the error path, one Trainer.train_batch on a loader
batch against the same tuple built per utterance, and Trainer.evaluate against the oracle.
Every wav is written here (at most 1 s)."""
import os
import random
import threading

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from ds2amd import model as dsm
from ds2amd.data_loader import (BucketingSampler, DeviceBatchLoader, Labels, SpectrogramDataset,
                                SpectrogramParser, _collate_fn, load_audio_norm)
from ds2amd.decoder import GreedyDecoder
from ds2amd.trainer import Trainer, get_cer_wer
from oracle import ds2_oracle as orc

pytestmark = pytest.mark.gpu

LABELS = orc.LABELS
CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
# frames 1 + n // 160: 51, 101, 76, 101 (a tie with utterance 1), 31; utterance 2 is stereo
FRAMES = [8000, 16000, 12000, 16050, 4800]
TEXTS = ["hello world", "a little book", "see the moon", "too good", "odd"]


def _manifest(tmp_path, frames=FRAMES, texts=TEXTS, stereo=(2,), seed=0):
    rng = np.random.default_rng(seed)
    rows = []
    for i, n in enumerate(frames):
        shape = (n, 2) if i in stereo else (n,)
        w = os.path.join(str(tmp_path), f"u{i}.wav")
        wavfile.write(w, 16000, (rng.standard_normal(shape) * 5000).astype(np.int16))
        t = os.path.join(str(tmp_path), f"u{i}.txt")
        with open(t, "w", encoding="utf8") as f:
            f.write(texts[i % len(texts)])
        rows.append((w, t))
    man = os.path.join(str(tmp_path), "manifest.csv")
    with open(man, "w", newline="") as f:
        f.writelines(f"{w},{t}\n" for w, t in rows)
    return man, rows


def _reader_threads():
    return [t for t in threading.enumerate() if t.name == "ds2-wav-reader"]


def _equal_batches(a, b):
    assert torch.equal(a[0].cpu(), b[0].cpu())
    assert torch.equal(a[1], b[1]) and a[2] == b[2]
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert a[3].dtype == torch.float32 and a[1].dtype == a[4].dtype == torch.int32


@pytest.fixture()
def setup(dev, tmp_path):
    man, rows = _manifest(tmp_path)
    ds = SpectrogramDataset(CONF, man, None, LABELS, normalize='max_frame', augment=False,
                            device=dev)
    sampler = BucketingSampler(ds, batch_size=5)
    np.random.seed(11)
    loader = DeviceBatchLoader(ds, sampler, prefetch=2)
    assert len(loader) == 1
    batches = list(loader)
    assert len(batches) == 1 and not _reader_threads()
    order = list(sampler.bins[0])          # the sampler shuffles its bin in place
    return ds, rows, order, batches[0]


def test_batch_vs_reference_collate_over_oracle_spectrograms(setup):
    ds, rows, order, batch = setup
    labels = Labels(LABELS)
    items = [(orc.spectrogram(load_audio_norm(rows[i][0])[0]),
              labels.parse(open(rows[i][1], encoding="utf8").read()), rows[i][0]) for i in order]
    ref = _collate_fn(items)
    inputs = batch[0].cpu()
    assert batch[0].is_cuda and inputs.shape == ref[0].shape == (5, 1, 161, 101)
    # row order, the tie included: sorted(..., reverse=True) is stable
    assert batch[2] == ref[2]
    fr = {rows[i][0]: 1 + n // 160 for i, n in enumerate(FRAMES)}
    assert [fr[p] for p in batch[2]] == [101, 101, 76, 51, 31]
    tie = [p for p in batch[2] if fr[p] == 101]
    assert tie == [rows[i][0] for i in order if FRAMES[i] >= 16000]
    for x, p in enumerate(batch[2]):
        t = fr[p]
        err = (inputs[x, 0, :, :t] - ref[0][x, 0, :, :t]).abs().max().item()
        print(f"row {x}: max abs err {err:.3e}")
        assert err < 2e-4, (x, err)               # test_stft_vs_oracle's bound
        assert inputs[x, 0, :, t:].abs().sum().item() == 0
    assert torch.equal(batch[1], ref[1]) and torch.equal(batch[4], ref[4])
    assert torch.equal(batch[3], ref[3]) and batch[3].dtype == torch.float32
    # the doubled letters went through the '2' rule
    assert labels.labels_map['2'] in batch[1].tolist()


def test_batch_equals_collate_over_getitem(setup):
    ds, rows, order, batch = setup
    ref = _collate_fn([ds[i] for i in order])
    _equal_batches(batch, ref)


def test_prefetch_does_not_change_a_seeded_augmented_run(dev, tmp_path):
    rng = np.random.default_rng(3)
    wavfile.write(os.path.join(str(tmp_path), "noise0.wav"), 16000,
                  (rng.standard_normal(16000) * 3000).astype(np.int16))
    man, rows = _manifest(tmp_path, frames=[3000, 8000, 5000, 6100, 4000, 7000, 3500], seed=1)
    conf = dict(CONF, noise_prob=0.6, noise_dir=os.path.join(str(tmp_path), "noise*.wav"),
                aug_prob_spect=0.5, aug_prob_8khz=0.3)
    runs = []
    for prefetch in (0, 2):
        # OneOf pins a chosen transform's prob for good and the sampler shuffles in place:
        # a fresh dataset and sampler per run
        ds = SpectrogramDataset(conf, man, None, LABELS, normalize='max_frame', augment=True,
                                device=dev)
        sampler = BucketingSampler(ds, batch_size=3)
        loader = DeviceBatchLoader(ds, sampler, prefetch=prefetch)
        random.seed(5)
        np.random.seed(5)
        torch.manual_seed(5)
        out = []
        for epoch in range(2):
            sampler.shuffle(epoch)
            out += list(loader)
        assert len(out) == 6 and not _reader_threads()
        runs.append(out)
    for a, b in zip(*runs):
        _equal_batches(a, b)
    # the two epochs are not one epoch twice: shuffle(epoch) and the draws moved on
    assert [b[2] for b in runs[0][:3]] != [b[2] for b in runs[0][3:]]


def test_parse_batch_draw_order_follows_the_sampler(dev):
    """The per-utterance draws (mask bands, 'max_frame' offset) made in draw_order: a batch
    whose rows were reordered, drawn in the original order, is the original batch with its
    rows reordered."""
    conf = dict(CONF, noise_prob=1.0, aug_prob_spect=1.0, aug_prob_8khz=0.5)
    parser = SpectrogramParser(conf, normalize='max_frame', augment=True, device=dev)
    rng = np.random.default_rng(8)
    sig = [(rng.standard_normal(n) * 0.3).astype(np.float32) for n in (4000, 9000, 2500, 6000)]
    perm = [1, 3, 0, 2]                                 # row x holds utterance perm[x]

    def run(signals, **kw):
        random.seed(6)
        np.random.seed(6)
        torch.manual_seed(6)
        return parser.parse_batch(signals, **kw)

    base, bf = run(sig)
    got, gf = run([sig[p] for p in perm], draw_order=[perm.index(p) for p in range(4)])
    assert torch.equal(gf, bf[perm]) and torch.equal(got, base[perm])
    plain, _ = run([sig[p] for p in perm])
    assert not torch.equal(plain, got)                  # row-by-row draws are another batch
    with pytest.raises(ValueError):
        parser.parse_batch(sig, draw_order=[0, 1, 2, 2])


def test_missing_wav_raises_with_its_path(dev, tmp_path):
    man, rows = _manifest(tmp_path)
    os.remove(rows[3][0])
    ds = SpectrogramDataset(CONF, man, None, LABELS, normalize='max_frame', device=dev)
    for prefetch in (0, 2):
        loader = DeviceBatchLoader(ds, BucketingSampler(ds, batch_size=2), prefetch=prefetch)
        with pytest.raises(RuntimeError, match="u3.wav"):
            list(loader)
        assert not _reader_threads()


def _tiny(seed=21):
    torch.manual_seed(seed)
    return dsm.DeepSpeech(rnn_type='gru', labels=LABELS, rnn_hidden_size=16, nb_layers=2,
                          audio_conf=CONF, bidirectional=True)


_POOL_STREAMS = [0]      # streams this module took from torch's pool (one per Trainer)


def _trainer(model, dev, **kw):
    _POOL_STREAMS[0] += 1                          # Trainer's decode side stream
    return Trainer(model, LABELS, device=dev, verbose=False, **kw)


@pytest.fixture(scope="module", autouse=True)
def _leave_stream_pool_where_it_was(dev):
    """torch hands out its 32 pooled streams per device round-robin, and which hardware queue
    a stream runs on follows from its place in the pool.  Tests that run later in the same
    process and time a side stream against the default stream (tests/test_gpu_residency.py)
    were written with the pool at a given place; this module takes the rest of a full turn
    so that they get the same stream with or without it."""
    yield
    for _ in range(-_POOL_STREAMS[0] % 32):
        torch.cuda.Stream(dev)


def test_train_batch_on_loader_batch_equals_per_utterance_tuple(setup, dev):
    """One step on the loader's batch == one step on the tuple built the old way
    (parse_audio per utterance through load_audio_norm, Labels.parse, _collate_fn; inputs
    on the host): loss and every parameter after the step, bit for bit."""
    ds, rows, order, batch = setup
    parser = SpectrogramParser(CONF, normalize='max_frame', device=dev)
    labels = Labels(LABELS)
    old = _collate_fn([(parser.parse_audio(rows[i][0]).cpu(),
                        labels.parse(open(rows[i][1], encoding="utf8").read()), rows[i][0])
                       for i in order])
    assert not old[0].is_cuda
    results = []
    for data in (batch, old):
        tr = _trainer(_tiny(), dev, lr=3e-4, momentum=0.9, max_norm=100.0)
        data = (data[0], data[1], data[2], data[3].clone(), data[4])
        loss = tr.train_batch(data, return_item=True)
        assert np.isfinite(loss)
        results.append((loss, {k: v.detach().cpu().clone()
                               for k, v in tr.model.state_dict().items()}))
    assert results[0][0] == results[1][0]
    for k, v in results[0][1].items():
        assert torch.equal(v, results[1][1][k]), k


def test_evaluate_vs_oracle(dev, tmp_path):
    """Trainer.evaluate over a 2-bin loader vs the oracle's eval forward, CTC, greedy decode
    and the host Decoder.wer / .cer: sums and counts exact; val_loss within the 1e-4 relative
    bound the train tests put on a loss (tests/test_gpu_train.py:267, :658; the eval-forward
    test bounds its logits by the same figure, :611)."""
    man, rows = _manifest(tmp_path)
    ds = SpectrogramDataset(CONF, man, None, LABELS, normalize='max_frame', device=dev)
    m = _tiny()
    o = orc.OracleDS2({k: v.detach().clone() for k, v in m.state_dict().items()}, 2, 16)
    tr = _trainer(m, dev)
    before = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}

    def loader():
        np.random.seed(2)
        return DeviceBatchLoader(ds, BucketingSampler(ds, batch_size=3), prefetch=2)

    assert len(loader()) == 2
    got = tr.evaluate(loader())
    assert tr.model.training
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v.cpu(), before[k]), k

    host = GreedyDecoder(LABELS)
    loss_sum, n_loss = 0.0, 0
    sums = [0.0, 0.0, 0.0, 0.0]
    for inputs, targets, _, pct, tsz in loader():
        x = inputs.cpu()
        sizes = orc.input_sizes_quirk(pct, x.size(3))
        with torch.no_grad():
            rl, rp, ro, _ = o.forward(x, sizes, training=False)
        loss, _ = orc.ctc_loss(rl.transpose(0, 1), targets, ro, tsz)
        v = float(loss) / x.size(0)
        assert np.isfinite(v)
        loss_sum = loss_sum * 0.998 + v * 0.002
        loss_sum += v
        n_loss += 1
        strings, _ = orc.greedy_decode(rp, ro.tolist())
        split, off = [], 0
        for s in tsz.tolist():
            split.append(targets[off:off + s])
            off += s
        refs = host.convert_to_strings(split)
        for a, b in zip(strings, refs):
            for j, q in enumerate(get_cer_wer(host, a[0], b[0])):
                sums[j] += q
    assert n_loss == 2
    assert got["num_words"] == sums[2] and got["num_chars"] == sums[3]
    assert got["wer"] == 100 * sums[0] / sums[2]
    assert got["cer"] == 100 * sums[1] / sums[3]
    ref_loss = loss_sum / n_loss
    print(f"val_loss {got['val_loss']!r} oracle {ref_loss!r}")
    assert abs(got["val_loss"] - ref_loss) <= 1e-4 * abs(ref_loss)

    # the best beam of a BeamCTCDecoder in place of the greedy path: same loss and reference
    # counts, error sums those of its own best strings
    from ds2amd.decoder import BeamCTCDecoder
    beam = BeamCTCDecoder(LABELS, beam_width=8)
    got_b = tr.evaluate(loader(), decoder=beam)
    assert tr.model.training
    assert got_b["val_loss"] == got["val_loss"]
    assert (got_b["num_words"], got_b["num_chars"]) == (sums[2], sums[3])
    bs = [0.0, 0.0]
    tr.model.eval()
    with torch.no_grad():
        for inputs, targets, _, pct, tsz in loader():
            _, probs, out_sizes = tr.model(inputs, pct.mul_(int(inputs.size(3))).int())
            strings, _ = beam.decode(probs, out_sizes)
            split, off = [], 0
            for s in tsz.tolist():
                split.append(targets[off:off + s])
                off += s
            for a, b in zip(strings, host.convert_to_strings(split)):
                w, c, _, _ = get_cer_wer(host, a[0], b[0])
                bs[0] += w
                bs[1] += c
    tr.model.train()
    assert got_b["wer"] == 100 * bs[0] / sums[2] and got_b["cer"] == 100 * bs[1] / sums[3]
