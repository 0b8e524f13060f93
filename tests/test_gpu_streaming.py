"""GPU: ds2amd.streaming.StreamingSession against the whole-utterance float64 oracle.

For any partition of a [N, 1, 161, T] spectrogram into chunks, the outputs of the feed calls
and of finish, concatenated over time, must be the eval forward of the whole utterance.  Truth
is oracle.ds2_oracle.OracleDS2.forward(training=False) with every tensor cast to float64; the
bound is the project's whole-model forward tolerance, 1e-4 of max |ref| on logits and probs
(tests/test_gpu_model.py).  With DS2_STREAM_PARITY_OUT naming a file, every comparison appends
the float32 oracle's, this library's whole-utterance and the streamed distance from that truth
(profiles/streaming_parity.txt is such a file).
"""
import os

import pytest
import torch

from ds2amd import model as dsm
from ds2amd.streaming import StreamingSession
from oracle import ds2_oracle as orc

pytestmark = pytest.mark.gpu

N, HIDDEN, LAYERS, CONTEXT = 2, 32, 2, 20
CONF = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming')
REL = 1e-4


def build(rnn_type, **kw):
    """seeded weights, non-trivial seeded BN running statistics, eval mode, on the CPU"""
    torch.manual_seed(11)
    args = dict(rnn_type=rnn_type, labels=orc.LABELS, rnn_hidden_size=HIDDEN, nb_layers=LAYERS,
                audio_conf=CONF, bidirectional=False, context=CONTEXT)
    args.update(kw)
    m = dsm.DeepSpeech(**args)
    g = torch.Generator().manual_seed(12)
    for mod in m.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.2)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return m.eval()


_CASES = {}


def case(dev, rnn_type, t):
    """(model on the device, x on the device, truth (logits, probs) float64, the float32
    oracle's and the whole-utterance forward's outputs): computed once, shared, never changed"""
    key = (rnn_type, t)
    if key not in _CASES:
        m = build(rnn_type)
        x = torch.randn(N, 1, 161, t, generator=torch.Generator().manual_seed(100 + t))
        lengths = torch.full((N,), t, dtype=torch.int32)
        o = orc.OracleDS2({k: v.detach().clone() for k, v in m.state_dict().items()}, LAYERS,
                          HIDDEN, bidirectional=False, rnn_type=rnn_type)
        with torch.no_grad():
            l32, p32, lens32, _ = o.forward(x, lengths, training=False)
            o.sd = {k: v.double() if v.is_floating_point() else v for k, v in o.sd.items()}
            l64, p64, lens64, _ = o.forward(x.double(), lengths, training=False,
                                            params=o.parameters())
        assert l64.dtype == torch.float64 and lens64.tolist() == [(t - 1) // 2 + 1] * N
        m = m.to(dev)
        xd = x.to(dev)
        with torch.no_grad():
            lw, pw, lens_w = m(xd, lengths)
        assert lens_w.cpu().tolist() == lens64.tolist()
        _CASES[key] = (m, xd, (l64, p64), (l32, p32), (lw.double().cpu(), pw.double().cpu()))
    return _CASES[key]


def dist(got, ref):
    return (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def partition(name, t):
    if name == "one":
        return [t]
    if name == "ones":
        return [1] * t
    if name == "mixed":
        head = [7, 1, 13, 2, 0]
        return head + [t - sum(head)]
    sizes = [1]
    while sum(sizes) < t:
        sizes.append(min(2, t - sum(sizes)))
    return sizes


@pytest.mark.parametrize("part", ["one", "ones", "mixed", "one-twos"])
@pytest.mark.parametrize("t", [75, 74, 24])
@pytest.mark.parametrize("rnn_type", ["gru", "lstm"])
def test_streamed_equals_whole_utterance(dev, rnn_type, t, part):
    m, x, truth, o32, whole = case(dev, rnn_type, t)
    t_out = (t - 1) // 2 + 1
    s = StreamingSession(m, n_streams=N)
    logits, probs, counts, seen = [], [], [], 0
    a = 0
    for size in partition(part, t):
        lg, pr = s.feed(x[..., a:a + size].contiguous())
        a += size
        seen += lg.shape[1]
        # output frame j is final only once input frame 2 (j + context) + 15 has arrived
        assert seen <= max(0, (a - 16) // 2 - CONTEXT + 1), (a, seen)
        assert lg.shape == pr.shape == (N, lg.shape[1], len(orc.LABELS))
        logits.append(lg)
        probs.append(pr)
        counts.append(lg.shape[1])
    assert a == t
    lg, pr = s.finish()
    logits.append(lg)
    probs.append(pr)
    counts.append(lg.shape[1])
    assert sum(counts) == t_out, counts
    if t_out < CONTEXT:
        assert counts[-1] == t_out      # everything arrives at finish
    with pytest.raises(RuntimeError):
        s.feed(x[..., :1].contiguous())
    got = (torch.cat(logits, 1), torch.cat(probs, 1))
    out = os.environ.get("DS2_STREAM_PARITY_OUT")
    errs = []
    for name, g_, ref, r32, rw in zip(("logits", "probs"), got, truth, o32, whole):
        d32, dw, ds = dist(r32, ref), dist(rw, ref), dist(g_, ref)
        print(f"{rnn_type} T={t} {part} {name}: oracle32 {d32:.3e} whole {dw:.3e} "
              f"streamed {ds:.3e}")
        if out:
            with open(out, "a") as f:
                f.write(f"{rnn_type} T={t} {part} {name} {d32:.3e} {dw:.3e} {ds:.3e}\n")
        errs.append((name, dw, ds))
    for name, dw, ds in errs:
        assert ds <= REL, f"{name}: streamed {ds:.3e} > {REL:.0e} (whole utterance {dw:.3e})"


def test_constructor_refusals(dev):
    with pytest.raises(ValueError):
        StreamingSession(build("gru", bidirectional=True).to(dev))
    with pytest.raises(ValueError):
        StreamingSession(build("rnn").to(dev))
    with pytest.raises(ValueError):
        StreamingSession(build("cnn", nb_layers=1).to(dev))
    with pytest.raises(ValueError):
        StreamingSession(build("lstm", rnn_gemm_precision='bf16').to(dev))
    with pytest.raises(ValueError):
        StreamingSession(build("gru").to(dev).train())
    StreamingSession(build("gru").to(dev), n_streams=3)


def test_finish_twice_and_empty(dev):
    s = StreamingSession(build("gru").to(dev), n_streams=N)
    lg, pr = s.finish()
    assert lg.shape == pr.shape == (N, 0, len(orc.LABELS))
    with pytest.raises(RuntimeError):
        s.finish()
