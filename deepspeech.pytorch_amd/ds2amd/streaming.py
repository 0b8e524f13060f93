"""Streaming (chunked) inference of a unidirectional DeepSpeech model.

``StreamingSession`` takes normalised spectrogram frames as they arrive and returns the output
frames that have become final; over any partition of an utterance the concatenated outputs are
the whole-utterance eval forward ``model(x, lengths=[T] * N)``.

What is carried between calls (a few small device tensors; all counts follow from the chunk
sizes on the host, so ``feed`` never synchronises):

* conv1 (time kernel 11, stride 2, pad 5): the input frames its next output still needs.  Its
  output j reads input frames 2j - 5 .. 2j + 5, so the window kept starts at frame 2j - 5 of
  the next j: odd chunk boundaries are held back until the stride-2 grid is respected.
* conv2 (time kernel 11, stride 1, pad 5): conv1's last 10 output frames.  Both convolutions
  run the existing conv block (conv -> BN on running statistics -> Hardtanh) on explicit
  windows with time padding 0; the zero padding exists only at the true start (five zero
  frames before frame 0) and, at ``finish``, at the true end -- for conv2 these are zeros of
  conv1's masked activation, not conv1 applied to zero input.
* every recurrent layer's state (h, and c for the LSTM): ops.gru_forward_state /
  ops.lstm_forward_state start each chunk from it.
* the Lookahead convolution's ``context`` last recurrent frames: output j needs frames
  j .. j + context, the kernel runs on [carried ++ new] and only outputs with full context are
  emitted; ``finish`` computes the rest with the kernel's own zeros past the end.

Hence output frame j is final once input frame 2 (j + context) + 15 has arrived: 55 input
frames (0.55 s at the 10 ms stride) of algorithmic latency at the default context of 20.

The probabilities go to ds2amd.decoder.StreamingGreedyDecoder or, for the prefix beam search
with the n-gram LM, to ds2amd.decoder.StreamingBeamCTCDecoder, chunk by chunk.

Out of scope: a streaming STFT (the session takes normalised frames; per-utterance mean / std
normalisation needs the whole utterance).
"""
from __future__ import annotations

import torch

from . import model as dsm
from . import ops

KT, PT = 11, 5      # time kernel and time padding of both convolutions


class StreamingSession:
    """``s = StreamingSession(model, n_streams=N)``; ``logits, probs = s.feed(chunk)`` with chunk
    [N, 1, 161, Tc] on the device (Tc >= 0) returns [N, k, C] for the k >= 0 frames that became
    final; ``s.finish()`` returns the frames still held back.  All N streams advance in
    lock-step and end together (streams that end at different times need several sessions).

    Output frame j is emitted by the call that delivers input frame 2 (j + context) + 15 (55
    frames of algorithmic latency at context 20), or by ``finish``.

    The model must be in eval mode, unidirectional ('gru' or 'lstm', with its Lookahead layer)
    and fp32 (rnn_gemm_precision='fp32'); anything else raises ValueError.
    """

    def __init__(self, model: dsm.DeepSpeech, n_streams: int = 1):
        if not isinstance(model, dsm.DeepSpeech):
            raise ValueError("StreamingSession needs a ds2amd DeepSpeech model")
        if model._rnn_type not in ('gru', 'lstm'):
            raise ValueError(f"StreamingSession: rnn_type {model._rnn_type!r} cannot stream "
                             "(recurrences with a carried state: 'gru', 'lstm')")
        if model._bidirectional or model.lookahead is None:
            raise ValueError("StreamingSession needs bidirectional=False: a backward direction "
                             "reads the whole utterance")
        if model._rnn_gemm_precision != 'fp32':
            raise ValueError("StreamingSession runs the fp32 recurrences "
                             "(rnn_gemm_precision='fp32')")
        if model.training:
            raise ValueError("StreamingSession needs model.eval(): BatchNorm on running statistics")
        if n_streams < 1:
            raise ValueError("n_streams >= 1")
        self.model = model
        self.n = int(n_streams)
        self.kind = model._rnn_type
        self.context = model.lookahead[0].context
        self.dev = next(model.parameters()).device
        if self.dev.type != 'cuda':
            raise RuntimeError("ds2amd.StreamingSession runs on the GPU only (HIP kernels)")
        c1 = model.conv.seq_module[0]
        self.freq = 161
        d1 = ops.conv_out_shape(self.freq, KT, c1.kernel_size[0], KT, c1.stride[0], 1,
                                c1.padding[0], 0)[0]
        f32 = dict(device=self.dev, dtype=torch.float32)
        # the true start: five zero frames in front of the input and of conv1's output
        self._in = torch.zeros(self.n, 1, self.freq, PT, **f32)
        self._c1 = torch.zeros(self.n, c1.out_channels, d1, PT, **f32)
        self._state = [None] * len(model.rnns)          # per layer: (h,) or (h, c)
        self._la = None                                 # recurrent frames without full context
        self.frames_in = 0                              # input frames taken so far
        self.frames_out = 0                             # output frames returned so far
        self._done = False

    # ---- the stages, each on the frames that are new to it -------------------------------
    def _conv_block(self, i, window, layout):
        """conv block i of MaskConv (3 i: conv, BN, Hardtanh) on an explicit window, time
        padding 0; every output frame is a real one (no mask inside a window)."""
        m = self.model.conv.seq_module
        conv, bn, act = m[3 * i], m[3 * i + 1], m[3 * i + 2]
        k = (window.shape[3] - KT) // conv.stride[1] + 1
        lens = ops._full_lens(k, self.n, self.dev)
        return ops.ConvBlockFn.apply(window, lens, conv.weight, conv.bias, bn.weight, bn.bias,
                                     bn.running_mean, bn.running_var, False, 0.0, bn.eps,
                                     tuple(conv.stride), (conv.padding[0], 0), act.min_val,
                                     act.max_val, layout)

    def _convs(self, chunk, last):
        """new input frames -> new conv2 frames [k, N, C D] (None when there is none yet)"""
        zeros = lambda like: like.new_zeros(*like.shape[:3], PT)
        parts = [self._in, chunk] + ([zeros(self._in)] if last else [])
        self._in = torch.cat(parts, 3)
        k1 = (self._in.shape[3] - KT) // 2 + 1 if self._in.shape[3] >= KT else 0
        new1 = []
        if k1 > 0:
            new1 = [self._conv_block(0, self._in, 0)]
            self._in = self._in[..., 2 * k1:].contiguous()
        parts = [self._c1] + new1 + ([zeros(self._c1)] if last else [])
        if len(parts) > 1:
            self._c1 = torch.cat(parts, 3)
        k2 = self._c1.shape[3] - (KT - 1)
        if k2 <= 0:
            return None
        y = self._conv_block(1, self._c1, 1)
        self._c1 = self._c1[..., k2:].contiguous()
        return y

    def _rnns(self, x):
        """[k, N, F] -> [k, N, H] through every recurrent layer from its carried state"""
        k = x.shape[0]
        fn = ops.gru_forward_state if self.kind == 'gru' else ops.lstm_forward_state
        for i, layer in enumerate(self.model.rnns):
            if layer.batch_norm is not None:
                x = layer.batch_norm(x)
            st = self._state[i] or ()
            x, *st = fn(x, k, layer.rnn._weights(), *st)
            self._state[i] = tuple(st)
        return x

    def _lookahead(self, x, last):
        """new recurrent frames -> the Lookahead + Hardtanh outputs that have full context (all
        of them at the end); None when there is none"""
        if x is not None:
            self._la = x if self._la is None else torch.cat([self._la, x], 0)
        if self._la is None:
            return None
        have = self._la.shape[0]
        k = have if last else have - self.context
        if k <= 0:
            return None
        la, ht = self.model.lookahead[0], self.model.lookahead[1]
        y = la.forward_htanh(self._la, ht.min_val, ht.max_val)[:k]
        self._la = self._la[k:] if k < have else None
        return y

    def _advance(self, chunk, last):
        with torch.no_grad():
            x = self._convs(chunk, last)
            if x is not None:
                x = self._rnns(x)
            x = self._lookahead(x, last)
            if x is None:
                c = self.model.fc[0].module[1].weight.shape[0]
                empty = torch.empty(self.n, 0, c, device=self.dev, dtype=torch.float32)
                return empty, empty.clone()
            x = self.model.fc(x.contiguous())                   # [k, N, C]
            probs = ops.SoftmaxTNCFn.apply(x)
        self.frames_out += x.shape[0]
        return x.transpose(0, 1), probs

    # ---- public ---------------------------------------------------------------------------
    def feed(self, chunk: torch.Tensor):
        """chunk [N, 1, 161, Tc], Tc >= 0, float32 on the model's device -> (logits, probs),
        both [N, k, C], k >= 0: the output frames this chunk made final."""
        if self._done:
            raise RuntimeError("StreamingSession.feed after finish(): start a new session")
        if chunk.dim() != 4 or tuple(chunk.shape[:3]) != (self.n, 1, self.freq):
            raise ValueError(f"chunk must be [{self.n}, 1, {self.freq}, Tc], got "
                             f"{tuple(chunk.shape)}")
        if not chunk.is_cuda or chunk.dtype != torch.float32:
            raise ValueError("chunk must be a float32 device tensor")
        self.frames_in += chunk.shape[3]
        return self._advance(chunk.detach(), False)

    def finish(self):
        """The frames still held back: the true end of the utterance (zero padding of both
        convolutions, the Lookahead's zeros past the end).  The session is closed afterwards."""
        if self._done:
            raise RuntimeError("StreamingSession.finish called twice")
        self._done = True
        if self.frames_in == 0:
            c = self.model.fc[0].module[1].weight.shape[0]
            empty = torch.empty(self.n, 0, c, device=self.dev, dtype=torch.float32)
            return empty, empty.clone()
        return self._advance(self._in.new_zeros(self.n, 1, self.freq, 0), True)
