"""GPU: the streaming front-end (csrc/stft_stream.hip, ds2amd.streaming.StreamingFrontend and
StreamingTranscriber).

'none' must be bit for bit the rows of ops.stft_logmag(normalize=0) on the whole utterance over
every partition, with the host's count of frames per feed.  The causal 'max_frame' must be bit
for bit the same over every partition and within stream_frontend_common's bound of the float64
restatement.  The C entry point runs on poisoned operands with a state and workspace of exactly
the queried bytes.  End to end, PCM chunks through StreamingTranscriber give the text and
offsets of the front-end's one-shot frames through StreamingSession and the decoder."""
import numpy as np
import pytest
import torch

from ds2amd import _lib, ops
from ds2amd import model as dsm
from ds2amd.decoder import StreamingBeamCTCDecoder, StreamingGreedyDecoder
from ds2amd.streaming import StreamingFrontend, StreamingSession, StreamingTranscriber
from oracle import ds2_oracle as orc

import frontend_common as fc
import stream_frontend_common as sc
from conv_common import Poisoned, Workspace

pytestmark = pytest.mark.gpu


def rows_of(n, n_streams, shift=0):
    """(kind, seed) per stream: the four kinds rotate with the length and the stream"""
    i = sc.LENGTHS.index(n) if n in sc.LENGTHS else 0
    return [(sc.KINDS[(i + s + shift) % len(sc.KINDS)], 900 + 7 * i + s) for s in range(n_streams)]


def pcm_of(n, rows, hop, dev):
    return torch.from_numpy(np.stack([fc.signal(kind, n, seed, hop) for kind, seed in rows])).to(dev)


def run(front, pcm, sizes, check_counts=True):
    """feed the chunks, finish -> [N, 161, T] and the frames per call (finish last)"""
    outs, a = [], 0
    for s in sizes:
        o = front.feed(pcm[:, a:a + s])
        if check_counts:
            assert o.shape == (pcm.shape[0], 1, 161, ops.stft_stream_frames(a, a + s, False,
                                                                            front.n_fft, front.hop))
        outs.append(o)
        a += s
    o = front.finish()
    if check_counts:
        assert o.shape[3] == ops.stft_stream_frames(a, a, True, front.n_fft, front.hop)
    outs.append(o)
    assert front.samples_in == a and front.frames_out == sum(o.shape[3] for o in outs)
    return torch.cat(outs, 3)[:, 0], [o.shape[3] for o in outs]


def whole(pcm, n_fft, hop, window):
    """ops.stft_logmag(normalize=0) of the whole utterances -> [N, 161, T]"""
    n = pcm.shape[1]
    lens = torch.full((pcm.shape[0],), n, dtype=torch.int32, device=pcm.device)
    return ops.stft_logmag(pcm, lens, n_fft, hop, window, 0, None, fc.frames_of(n, n_fft, hop))


GRID = [(g, ns, n) for g in sc.GPU_GEOMETRIES for ns in (1, 3) for n in sc.LENGTHS]
GRID_IDS = [f"{g[0]}_{g[1]}-s{ns}-n{n}" for g, ns, n in GRID]


@pytest.mark.parametrize("geom,n_streams,n", GRID, ids=GRID_IDS)
def test_none_is_the_whole_utterance_bit_for_bit(dev, geom, n_streams, n):
    n_fft, hop = geom
    pcm = pcm_of(n, rows_of(n, n_streams), hop, dev)
    front = StreamingFrontend(sc.CONFS[geom], n_streams=n_streams, normalize='none', device=dev)
    assert (front.n_fft, front.hop) == geom
    want = whole(pcm, n_fft, hop, front._window)
    for name, sizes in sc.partitions(n, n_fft, hop).items():
        front.reset()
        got, _ = run(front, pcm, sizes)
        assert got.shape == want.shape, name
        assert torch.equal(got, want), (name, (got - want).abs().max().item())


@pytest.mark.parametrize("geom,n_streams,n", GRID, ids=GRID_IDS)
def test_causal_max_frame(dev, geom, n_streams, n):
    """Bit for bit the same over every partition; against the float64 restatement within
    4 e_ref + one float32 ulp of the largest |value|; silence gives minus the offset (zero
    without a prior), finite."""
    n_fft, hop = geom
    rows = rows_of(n, n_streams, shift=1)
    pcm = pcm_of(n, rows, hop, dev)
    front = StreamingFrontend(sc.CONFS[geom], n_streams=n_streams, device=dev)
    base = None
    for name, sizes in sc.partitions(n, n_fft, hop).items():
        front.reset()
        got, _ = run(front, pcm, sizes)
        if base is None:
            base, off = got, front.offset()
        else:
            assert torch.equal(got, base), name
            assert torch.equal(front.offset(), off), name
    assert torch.isfinite(base).all()
    host = base.cpu().numpy().astype(np.float64)
    for s, (kind, seed) in enumerate(rows):
        r = sc.causal_refs(kind, n, seed, n_fft, hop)
        err = np.abs(host[s] - r.ref).max()
        print(f"STREAM_FRONTEND {geom} n={n} {kind}: err / bound = {err / r.bound:.3f} "
              f"(e_ref {r.e_ref:.2e})")
        assert err <= r.bound, (kind, err, r.bound)
        assert abs(off[s].item() - r.off[-1]) <= r.bound
        if kind == "silence":
            assert not base[s].any()


@pytest.mark.parametrize("geom", sc.GPU_GEOMETRIES, ids=lambda g: f"{g[0]}_{g[1]}")
def test_prior_reset_and_fixed_offset(dev, geom):
    n_fft, hop = geom
    n, kinds = 1281, [("ramp", 31), ("silence", 32), ("impN", 33)]
    pcm = pcm_of(n, kinds, hop, dev)
    parts = sc.partitions(n, n_fft, hop)
    # a prior from the constructor: one (o0, w) for every stream
    prior = (6.5, 12.0)
    front = StreamingFrontend(sc.CONFS[geom], n_streams=3, prior=prior, device=dev)
    assert torch.equal(front.offset().cpu(), torch.full((3,), 6.5, dtype=torch.float64))
    got, _ = run(front, pcm, parts["mixed"])
    host = got.cpu().numpy().astype(np.float64)
    for s, (kind, seed) in enumerate(kinds):
        r = sc.causal_refs(kind, n, seed, n_fft, hop, prior)
        assert np.abs(host[s] - r.ref).max() <= r.bound, kind
        if kind == "silence":      # val = 0: the output is minus the offset, the prior decaying
            assert np.isfinite(host[s]).all() and np.abs(host[s] + r.off[None, :]).max() <= r.bound
            assert host[s].max() < 0
    # offset() is the utterance's own running mean (no prior in it); reset(prior=(offset(), w))
    # starts the next utterance from it, per stream, and is honoured over another partition
    o = front.offset()
    for s, (kind, seed) in enumerate(kinds):
        r0 = sc.causal_refs(kind, n, seed, n_fft, hop)
        assert abs(o[s].item() - r0.off[-1]) <= r0.bound
    pcm2 = pcm_of(n, [(k, sd + 10) for k, sd in kinds], hop, dev)
    front.reset(prior=(o, 5.0))
    assert torch.equal(front.offset(), o)
    a, _ = run(front, pcm2, parts["zero"])
    front.reset(prior=(o, 5.0))
    b, _ = run(front, pcm2, parts["all"])
    assert torch.equal(a, b)
    host = a.cpu().numpy().astype(np.float64)
    for s, (kind, seed) in enumerate(kinds):
        r = sc.causal_refs(kind, n, seed + 10, n_fft, hop, (o[s].item(), 5.0))
        assert np.abs(host[s] - r.ref).max() <= r.bound, kind
    front.reset()
    assert not front.offset().any()
    # a fixed offset: out + offset is val = log1p(|X| 2^20), the values the causal run subtracts
    # its offsets from.  offset 0 returns val itself; the causal output is val minus an offset
    # per frame, the same for all 161 rows, that is the restatement's
    zero = StreamingFrontend(sc.CONFS[geom], n_streams=3, offset=0.0, device=dev)
    val, _ = run(zero, pcm, parts["mixed"])
    fixed_by = torch.tensor([2.25, -1.5, 17.0], device=dev)
    fixed = StreamingFrontend(sc.CONFS[geom], n_streams=3, offset=fixed_by, device=dev)
    for name in ("all", "mixed"):
        fixed.reset()
        out, _ = run(fixed, pcm, parts[name])
        assert torch.equal(out, val - fixed_by[:, None, None]), name
    assert torch.equal(fixed.offset(), zero.offset())      # the running mean is kept all the same
    causal = StreamingFrontend(sc.CONFS[geom], n_streams=3, device=dev)
    c, _ = run(causal, pcm, parts["f789"] if "f789" in parts else parts["all"])
    sub = (val - c).cpu().numpy().astype(np.float64)             # the offsets it subtracted
    hv = val.cpu().numpy().astype(np.float64)
    for s, (kind, seed) in enumerate(kinds):
        r = sc.causal_refs(kind, n, seed, n_fft, hop)
        assert np.abs(hv[s] - r.val).max() <= r.val_bound, kind
        assert np.abs(sub[s] - r.off[None, :]).max() <= r.bound + r.val_bound, kind
    with pytest.raises(ValueError):
        fixed.reset(prior=(1.0, 1.0))


@pytest.mark.parametrize("normalize", ["none", "max_frame"])
def test_int16_input_is_the_float_input(dev, normalize):
    n, geom = 1281, (320, 160)
    g = torch.Generator().manual_seed(5)
    s16 = torch.randint(-32768, 32768, (3, n), generator=g, dtype=torch.int32).to(torch.int16)
    s16[0, :4] = torch.tensor([-32768, 32767, 0, -1], dtype=torch.int16)
    as_float = (s16.float() * 2.0 ** -15).to(dev)
    s16 = s16.to(dev)
    a = StreamingFrontend(sc.CONFS[geom], n_streams=3, normalize=normalize, device=dev)
    b = StreamingFrontend(sc.CONFS[geom], n_streams=3, normalize=normalize, device=dev)
    parts = sc.partitions(n, *geom)
    got16, _ = run(a, s16, parts["mixed"])
    gotf, _ = run(b, as_float, parts["zero"])
    assert torch.equal(got16, gotf)
    if normalize == "none":
        assert torch.equal(gotf, whole(as_float, *geom, a._window))
    # a row stride above the chunk (a view into a longer buffer) reads the same samples
    a.reset()
    wide = torch.zeros(3, n + 37, dtype=torch.int16, device=dev)
    wide[:, :n] = s16
    assert torch.equal(run(a, wide[:, :n], parts["mixed"])[0], got16)


def test_refusals_of_the_public_classes(dev):
    f = StreamingFrontend(sc.CONFS[(320, 160)], n_streams=2, device=dev)
    with pytest.raises(ValueError):
        f.feed(torch.zeros(2, 100))                                   # a host tensor
    with pytest.raises(ValueError):
        f.feed(torch.zeros(3, 100, device=dev))                       # another stream count
    with pytest.raises(ValueError):
        f.feed(torch.zeros(2, 100, device=dev, dtype=torch.float64))
    assert f.finish().shape == (2, 1, 161, 0)                         # finish without input
    with pytest.raises(RuntimeError):
        f.feed(torch.zeros(2, 100, device=dev))
    with pytest.raises(RuntimeError):
        f.finish()
    f.reset()
    assert f.feed(torch.zeros(2, 0, device=dev)).shape == (2, 1, 161, 0)
    assert f.feed(torch.zeros(2, 100, device=dev)).shape == (2, 1, 161, 0)
    assert f.finish().shape == (2, 1, 161, 1)                         # n <= pad: all at finish


# ------------------------------------------------------------------------------------------
# the C entry point on poisoned operands

class _Direct:
    """ds2_stft_stream_* called directly: the state and every feed's workspace are exactly the
    queried bytes inside canary allocations, the chunk lies in NaN, out in canaries."""

    def __init__(self, n, n_fft, hop, dev, normalize):
        self.n, self.n_fft, self.hop, self.dev, self.normalize = n, n_fft, hop, dev, normalize
        self.state = Workspace(_lib.size("ds2_stft_stream_state_size", n, n_fft, hop), dev)
        self.window = torch.from_numpy(orc.hamming(n_fft)).to(dev)
        self.frames = torch.full((n,), -7, dtype=torch.int32, device=dev)
        self.done = 0
        _lib.call("ds2_stft_stream_init", self.state.ptr, self.state.nbytes, n, n_fft, hop, None,
                  0.0, None)

    def feed(self, chunk, last, n_fft=None, hop=None, k=None, state_bytes=None):
        """chunk: a host [n, s] float tensor -> (status, out Poisoned or None, workspace)"""
        n_fft, hop = n_fft or self.n_fft, hop or self.hop
        s = chunk.shape[1]
        want = ops.stft_stream_frames(self.done, self.done + s, last, n_fft, hop)
        k = want if k is None else k
        stride = s + 3
        host = torch.full((self.n, stride), float("nan"))
        host[:, :s] = chunk
        pcm = Poisoned(host, self.dev)
        out = Poisoned((self.n, 161, max(k, 1)), self.dev) if k >= 0 else None
        ws = Workspace(_lib.size("ds2_stft_stream_workspace_size", self.n, max(k, 0)), self.dev)
        st = _lib.load().ds2_stft_stream_feed(
            pcm.ptr, 0, self.n, s, stride, 1.0, self.done, int(last), n_fft, hop,
            self.window.data_ptr(), self.normalize, None, out.ptr, k, None,
            self.frames.data_ptr(), self.state.ptr,
            self.state.nbytes if state_bytes is None else state_bytes, ws.ptr, ws.nbytes, None)
        torch.cuda.synchronize()
        assert self.state.intact() and ws.intact() and out.intact()
        if st == fc.OK and self.frames[0].item() >= 0:
            self.done += s
        return st, out, k


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("geom", sc.GPU_GEOMETRIES, ids=lambda g: f"{g[0]}_{g[1]}")
def test_entry_point_on_poisoned_operands(dev, geom, normalize):
    n_fft, hop = geom
    n, rows = 3601, [("ramp", 51), ("impN", 52)]       # every frame of "fssf" and a remainder
    pcm = pcm_of(n, rows, hop, dev)
    front = StreamingFrontend(sc.CONFS[geom], n_streams=2, device=dev,
                              normalize="max_frame" if normalize else "none")
    want, _ = run(front, pcm, [n])
    for name in ("mixed", "zero", "fssf"):
        sizes = sc.partitions(n, n_fft, hop)[name]
        d = _Direct(2, n_fft, hop, dev, normalize)
        outs, a = [], 0
        host = pcm.cpu()
        for i, s in enumerate(sizes + [0]):
            st, out, k = d.feed(host[:, a:a + s], last=i == len(sizes))
            assert st == fc.OK
            a += s
            if k > 0:
                outs.append(out.read())
        got = torch.cat(outs, 2)
        assert not torch.isnan(got).any(), name        # NaN lies past every chunk's samples
        assert torch.equal(got, want.cpu()), name
        assert d.frames.tolist() == [want.shape[2]] * 2


def test_refused_feeds_leave_everything_as_it_was(dev):
    """A wrong k and a too-small state are refused on the host; a record initialised for
    another geometry or another sample count is refused on the device (the tag lives there):
    frames -1, nothing written to out, the state unchanged."""
    d = _Direct(2, 320, 160, dev, 1)
    chunk = torch.from_numpy(np.stack([fc.signal("ramp", 400, 70 + i) for i in range(2)]))
    st, _, _ = d.feed(chunk[:, :200], last=False)
    assert st == fc.OK and d.frames.tolist() == [1, 1] and d.done == 200
    before = d.state.buf.clone()

    def untouched(out):
        return bool(torch.isnan(out.read()).all()) and torch.equal(d.state.buf, before)

    for k in (0, 2):                                   # 200 more samples complete one frame
        st, out, _ = d.feed(chunk[:, 200:], last=False, k=k)
        assert st == fc.INVALID_VALUE and untouched(out)
    st, out, _ = d.feed(chunk[:, 200:], last=False, state_bytes=d.state.nbytes - 1)
    assert st == fc.INVALID_VALUE and untouched(out)
    # hop 80 on a record of hop 160: the same state size, another tag
    assert _lib.size("ds2_stft_stream_state_size", 2, 320, 80) == d.state.nbytes
    st, out, _ = d.feed(chunk[:, 200:], last=False, hop=80)
    assert st == fc.OK and d.frames.tolist() == [-1, -1] and untouched(out)
    # the right geometry with a sample count the record has not reached
    d.done = 120
    st, out, _ = d.feed(chunk[:, 200:280], last=False)
    assert st == fc.OK and d.frames.tolist() == [-1, -1] and untouched(out)
    d.done = 200
    st, out, k = d.feed(chunk[:, 200:], last=False)
    assert st == fc.OK and k == 1 and d.frames.tolist() == [2, 2]
    assert not torch.isnan(out.read()).any() and not torch.equal(d.state.buf, before)


# ------------------------------------------------------------------------------------------
# end to end: the tiny unidirectional GRU of test_gpu_streaming.py

HIDDEN, LAYERS, CONTEXT = 32, 2, 20
E2E_CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')


def build_model(dev):
    """seeded weights, non-trivial seeded BN running statistics, eval mode"""
    torch.manual_seed(11)
    m = dsm.DeepSpeech(rnn_type='gru', labels=orc.LABELS, rnn_hidden_size=HIDDEN,
                       nb_layers=LAYERS, audio_conf=E2E_CONF, bidirectional=False, context=CONTEXT)
    g = torch.Generator().manual_seed(12)
    for mod in m.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return m.eval().to(dev)


E2E_CHUNKS = [6400, 159, 1, 0, 1600, 161, 2560, 3519]          # 6400 + 8000 samples


@pytest.mark.parametrize("which", ["greedy", "beam10"])
def test_transcriber_is_frontend_session_decoder(dev, which):
    assert sum(E2E_CHUNKS) == 6400 + 8000
    n = 2
    model = build_model(dev)
    pcm = pcm_of(sum(E2E_CHUNKS), [("ramp", 81), ("tone", 82)], 160, dev) * 0.1
    make = ((lambda: StreamingGreedyDecoder(orc.LABELS)) if which == "greedy" else
            (lambda: StreamingBeamCTCDecoder(orc.LABELS, beam_width=10, max_frames=200)))
    # the reference chain: one-shot frames -> session -> decoder
    front = StreamingFrontend(E2E_CONF, n_streams=n, device=dev)
    frames = torch.cat([front.feed(pcm), front.finish()], 3)
    assert frames.shape == (n, 1, 161, 91)
    session, dec = StreamingSession(model, n_streams=n), make()
    _, p1 = session.feed(frames)
    _, p2 = session.finish()
    want_last = dec.feed(torch.cat([p1, p2], 1))
    want_text = dec.text()
    # PCM chunks through the transcriber
    t = StreamingTranscriber(model, make(), n_streams=n)
    assert (t.frontend.n_fft, t.frontend.hop) == (320, 160)
    deltas, a = [], 0
    for s in E2E_CHUNKS:
        deltas.append(t.feed(pcm[:, a:a + s]))
        a += s
    deltas.append(t.finish())
    assert t.text() == want_text
    assert t.session.frames_in == 91 and t.session.frames_out == 46
    if which == "greedy":
        for b in range(n):
            assert "".join(d[0][b][0] for d in deltas) == want_text[b] == want_last[0][b][0]
            offs = torch.cat([d[1][b][0] for d in deltas])
            assert torch.equal(offs, want_last[1][b][0])
    else:
        strings, offsets = deltas[-1]          # the beam decoder returns the hypotheses in full
        assert strings == want_last[0]
        for b in range(n):
            assert torch.equal(offsets[b][0], want_last[1][b][0])
