"""CTC loss with the warpctc_pytorch.CTCLoss interface (ref train.py:12,904,600-602).

``CTCLoss()(acts[T,N,C], labels int32 flat, act_lens int32[N], label_lens int32[N])``
returns the summed cost as a 1-element tensor on the activations' device (warp-ctc
returns it on the host; the caller's ``loss.to(device)`` is then a no-op and no
host sync is forced).  Softmax is applied inside; the gradient is taken with
respect to the unnormalised activations and is produced by the same kernel launch
as the cost (ds2_ctc_loss).

Infeasible samples (more required frames than act_len): cost +inf and zero
gradient, or cost 0 with ``zero_infinity=True``.  warp-ctc's own behaviour for
them is not pinned by any reference test.

``forced_align`` takes the same four arguments and returns the best alignment of the
known labels to the frames (ds2_ctc_align) instead of a loss.
"""
from __future__ import annotations

import torch

from . import ops


class CTCLoss(torch.nn.Module):
    def __init__(self, blank=0, size_average=False, length_average=False, zero_infinity=False):
        super().__init__()
        self.blank = blank
        self.size_average = size_average
        self.length_average = length_average
        self.zero_infinity = zero_infinity

    def forward(self, acts, labels, act_lens, label_lens):
        if not acts.is_cuda:
            raise RuntimeError("ds2amd CTCLoss runs on the GPU (HIP kernel)")
        dev = acts.device
        label_lens_h = label_lens.cpu().int() if label_lens.is_cuda else label_lens.int()
        max_l = int(label_lens_h.max()) if label_lens_h.numel() else 0
        labels_d = labels.to(dev, torch.int32, non_blocking=True).contiguous()
        act_lens_d = act_lens.to(dev, torch.int32, non_blocking=True).contiguous()
        label_lens_d = label_lens_h.to(dev, non_blocking=True).contiguous()
        c = acts.shape[2]
        if labels.numel() and not labels.is_cuda:   # host labels (the reference's case)
            lo, hi = int(labels.min()), int(labels.max())
            if lo < 0 or hi >= c:
                raise ValueError(f"CTC labels must lie in [0, {c}), got [{lo}, {hi}]")
        loss = ops.CTCLossFn.apply(acts, labels_d, act_lens_d, label_lens_d, max_l, self.blank,
                                   self.zero_infinity, self.size_average)
        if self.length_average:
            loss = loss / max(1, int(label_lens_h.sum()))
        return loss.reshape(1)


class Alignment(object):
    """Result of `forced_align` (device tensors).

    states        int32 [N, T]: the extended CTC state per frame (even: blank, odd s: label
                  s >> 1 of the utterance), -1 beyond the utterance's length and everywhere
                  for an utterance whose labels do not fit its frames
    frame_labels  int32 [N, T]: the label id per frame (the blank on even states), -1 where
                  states is -1
    spans         list of N int32 [L_b, 2] tensors: per label its first frame and one past its
                  last (-1 for an utterance that does not fit)
    scores        float32 [N]: log-probability of the alignment (-inf where it does not fit)
    """

    def __init__(self, states, frame_labels, spans, scores):
        self.states = states
        self.frame_labels = frame_labels
        self.spans = spans
        self.scores = scores


def forced_align(acts, labels, act_lens, label_lens, blank=0):
    """Best CTC alignment (Viterbi) of each utterance's known labels to its frames, on the HIP
    kernel ds2_ctc_align.  Arguments as `CTCLoss.forward`: acts [T, N, C] unnormalised, labels
    flat int32, act_lens / label_lens [N], on the host or the device.  Not differentiable.
    Ties are broken as include/ds2hip.h states."""
    if not acts.is_cuda:
        raise RuntimeError("ds2amd forced_align runs on the GPU (HIP kernel)")
    dev = acts.device
    label_lens_h = label_lens.cpu().int() if label_lens.is_cuda else label_lens.int()
    max_l = int(label_lens_h.max()) if label_lens_h.numel() else 0
    c = acts.shape[2]
    if labels.numel() and not labels.is_cuda:
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= c:
            raise ValueError(f"CTC labels must lie in [0, {c}), got [{lo}, {hi}]")
    labels_d = labels.to(dev, torch.int32, non_blocking=True).contiguous()
    act_lens_d = act_lens.to(dev, torch.int32, non_blocking=True).contiguous()
    label_lens_d = label_lens_h.to(dev, non_blocking=True).contiguous()
    states, spans, scores = ops.ctc_align_raw(acts.detach().float(), labels_d, act_lens_d,
                                              label_lens_d, max_l, blank)
    # frame labels: a gather of each utterance's labels at states >> 1 on the device
    t = states.shape[1]
    offs = (torch.cumsum(label_lens_d, 0) - label_lens_d).long()
    odd = (states >= 0) & (states % 2 == 1)
    idx = (offs[:, None] + states.clamp(min=0) // 2).clamp(max=max(labels_d.numel() - 1, 0))
    if labels_d.numel() and t:
        lab = labels_d[idx.reshape(-1)].reshape(states.shape)
    else:
        lab = torch.full_like(states, int(blank))
    frame_labels = torch.where(odd, lab, torch.full_like(states, int(blank)))
    frame_labels = torch.where(states >= 0, frame_labels, torch.full_like(states, -1))
    per_utt = list(torch.split(spans, label_lens_h.tolist(), dim=0))
    return Alignment(states, frame_labels, per_utt, scores)
