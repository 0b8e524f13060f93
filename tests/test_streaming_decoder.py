"""GPU (the greedy kernel): StreamingGreedyDecoder over chunks equals GreedyDecoder.decode on
the whole tensor -- strings and absolute frame offsets -- where a repeated label, a
blank-separated repeat, a leading blank and a trailing blank all straddle chunk edges."""
import pytest
import torch

from ds2amd.decoder import GreedyDecoder, StreamingGreedyDecoder

pytestmark = pytest.mark.gpu

LABELS = "_abc "     # blank first; the space label is index 4

# per stream the argmax label of every frame (0 = blank).  With chunks of 2 the edges fall after
# frames 1, 3, 5, ...; with chunks of 1 after every frame.
#  stream 0: leading blank; a repeated over frames 1-3, across the edge 1|2 (one a); then the
#            blank-separated repeat a _ a over frames 3|4 5 (a second a); a trailing blank
#  stream 1: no leading blank; b repeated over three chunks; c _ | _ c (blank pair across an
#            edge); ends on a label repeated across the last edge; a space label
#  stream 2: all blank
FRAMES = [[0, 1, 1, 1, 0, 1, 2, 2, 0, 0, 3, 0],
          [2, 2, 2, 2, 2, 3, 0, 0, 3, 4, 1, 1],
          [0] * 12]


def one_hot(dev):
    idx = torch.tensor(FRAMES, device=dev)
    p = torch.full((len(FRAMES), idx.shape[1], len(LABELS)), 0.01, device=dev)
    return p.scatter_(2, idx[..., None], 0.96)


@pytest.mark.parametrize("chunk", [1, 2, 5, 12])
def test_chunked_greedy_equals_whole(dev, chunk):
    probs = one_hot(dev)
    n, t, _ = probs.shape
    want_s, want_o = GreedyDecoder(LABELS).decode(probs)
    assert [s[0] for s in want_s] == ["aabc", "bcc a", ""]       # the cases are what they claim
    d = StreamingGreedyDecoder(LABELS)
    got_s = [""] * n
    got_o = [[] for _ in range(n)]
    for a in range(0, t, chunk):
        s_, o_ = d.feed(probs[:, a:a + chunk])
        for b in range(n):
            got_s[b] += s_[b][0]
            got_o[b] += o_[b][0].tolist()
    s_, o_ = d.feed(probs[:, :0])                                  # an empty chunk adds nothing
    assert [s[0] for s in s_] == [""] * n and all(len(o[0]) == 0 for o in o_)
    assert got_s == [s[0] for s in want_s] == d.text()
    assert got_o == [o[0].tolist() for o in want_o]
