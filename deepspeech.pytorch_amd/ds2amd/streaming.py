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

The frames come from ``StreamingFrontend``: PCM chunks in, the spectrogram frames that have
become final out (csrc/stft_stream.hip, the per-frame code of the whole-utterance STFT).  With
a samples arrived frame t is final once max(t hop - pad + n_fft - 1, pad - t hop) <= a - 1, so
the front-end adds one frame (half a window, 10 ms at the defaults) to the 55 above.
``normalize='none'`` is bit for bit the whole-utterance ``log1p(|X|)``.  ``'max_frame'``
subtracts one scalar per utterance in the reference, ``mean_t(gauss20(mean_f))``, which needs
the whole utterance; a stream subtracts either a fixed ``offset=`` the caller already has (a
second pass, a calibrated channel) or, by default, the causal running mean of the frame means
``off_t = (w o0 + S_t) / (w + t + 1)`` with an optional prior ``(o0, w)`` -- a pure function of
the prefix, so partition-invariant bit for bit, but not the reference's scalar.  The reference
jitters that scalar by U(-0.5, 0.5) in training and at transcription (data_loader_aug.py:213-214,
transcribe.py:93-94); the causal mean comes within 0.5 of it after 0-4 frames on steady signals
and after 170 frames on a 3 s amplitude ramp.  The effect of the causal offset on WER has not
been measured: no parity with 'max_frame' is claimed.  Peak normalisation of the waveform
(load_audio_norm) is whole-utterance too; a gain g moves log1p(g S 2^20) by about log g where
S 2^20 >> 1, which the offset should absorb (supposed, not measured).

``StreamingTranscriber`` chains the three stages: PCM chunks in, text out.

Out of scope: the normalisations 'mean', 'norm' and 'frame' (whole-utterance statistics),
sample rates whose n_fft has fewer than 161 bins (the reference's mirror-fill reads frames
ahead of the column it fills), and the spectrogram masks (training augmentations).
"""
from __future__ import annotations

import torch

from . import model as dsm
from . import ops

KT, PT = 11, 5      # time kernel and time padding of both convolutions


class StreamingFrontend:
    """``f = StreamingFrontend(audio_conf, n_streams=N)``; ``frames = f.feed(pcm)`` with pcm
    [N, S] on the device (S >= 0; float32 in [-1, 1], or int16 read as s * 2^-15) returns
    [N, 1, 161, k], the k >= 0 spectrogram frames that became final -- ``StreamingSession.feed``'s
    input; ``f.finish()`` returns the frames up to librosa's count, reflected at the true end.
    All N streams advance in lock-step.  Counts are kept on the host: nothing synchronises.

    normalize: 'none' (log1p(|X|), bit for bit ``ops.stft_logmag(normalize=0)`` of the whole
    utterance) or 'max_frame' (log1p(|X| 2^20) minus an offset): ``offset=`` a float or [N]
    tensor subtracts that fixed value; without it the causal running mean of the frame means
    is subtracted, ``prior=(o0, w)`` (o0 a float or [N] tensor, w >= 0 frames) starting it from
    an earlier estimate.  ``offset()`` returns the running mean S_t / (t + 1) per stream
    (float64 [N] on the device), ``reset(prior=(f.offset(), w))`` starts the next utterance from
    it.  The causal offset is not the reference's whole-utterance scalar and its effect on WER
    is unmeasured (module docstring).  Other modes, and an n_fft with fewer than 161 or more
    than 256 bins, raise ValueError."""

    MODES = {'none': 0, 'max_frame': 1}

    def __init__(self, audio_conf, n_streams: int = 1, normalize='max_frame', offset=None,
                 prior=None, device='cuda'):
        from .data_loader import SpectrogramParser, windows
        if not normalize:
            normalize = 'none'
        if normalize not in self.MODES:
            known = sorted(SpectrogramParser.NORM_MODES)
            if normalize in known:
                raise ValueError(f"StreamingFrontend: normalize={normalize!r} needs statistics of "
                                 "the whole utterance; a stream has 'none' and 'max_frame'")
            raise ValueError(f"normalize={normalize!r}: the reference's modes are {known}")
        if n_streams < 1:
            raise ValueError("n_streams >= 1")
        sr = audio_conf['sample_rate']
        # n_fft, hop and the window as SpectrogramParser._consts takes them
        self.n_fft = int(sr * (audio_conf['window_size'] + 1e-8))
        self.hop = int(sr * (audio_conf['window_stride'] + 1e-8))
        bins = self.n_fft // 2 + 1
        if bins < ops.SPECT_ROWS:
            raise ValueError(f"StreamingFrontend: n_fft {self.n_fft} has {bins} bins; the "
                             "reference's mirror-fill to 161 rows reads frames ahead of the "
                             "column it fills and cannot be streamed")
        if self.n_fft > 1024 or bins > 256 or self.hop < 1:
            raise ValueError(f"StreamingFrontend: n_fft {self.n_fft} / hop {self.hop}: the STFT "
                             "kernels take n_fft <= 1024, n_fft // 2 + 1 <= 256 and hop >= 1")
        self.mode = self.MODES[normalize]
        if self.mode == 0 and (offset is not None or prior is not None):
            raise ValueError("StreamingFrontend: offset= and prior= belong to normalize='max_frame'")
        if offset is not None and prior is not None:
            raise ValueError("StreamingFrontend: a fixed offset= has no prior=")
        self.n = int(n_streams)
        self.dev = torch.device(device)
        if self.dev.type != 'cuda':
            raise ValueError("ds2amd.StreamingFrontend runs on the GPU only (HIP kernels)")
        win_fn = windows.get(audio_conf.get('window', 'hamming'), windows['hamming'])
        self._window = torch.tensor(win_fn(self.n_fft), dtype=torch.float64, device=self.dev)
        self._fixed = None
        if offset is not None:
            self._fixed = self._per_stream(offset, torch.float32)
        self._cur = torch.zeros(self.n, dtype=torch.float64, device=self.dev)
        self._state = None
        self.reset(prior)

    def _per_stream(self, v, dtype):
        if torch.is_tensor(v):
            if not v.is_cuda:
                raise ValueError("StreamingFrontend: offsets are floats or device tensors")
            v = v.detach().to(device=self.dev, dtype=dtype).reshape(-1)
            if v.numel() == 1:
                v = v.expand(self.n)
            if v.numel() != self.n:
                raise ValueError(f"StreamingFrontend: an offset per stream ([{self.n}])")
            return v.contiguous()
        return torch.full((self.n,), float(v), dtype=dtype, device=self.dev)

    def reset(self, prior=None):
        """Every stream back at the start of an utterance, in the same buffers.  prior: None or
        (o0, w) for the causal offset."""
        if prior is not None:
            if self.mode == 0 or self._fixed is not None:
                raise ValueError("StreamingFrontend: prior= belongs to the causal offset of "
                                 "normalize='max_frame'")
            o0, w = prior
            if not float(w) >= 0.0:
                raise ValueError("StreamingFrontend: prior weight w >= 0")
            prior = (self._per_stream(o0, torch.float64), float(w))
        self._state = ops.stft_stream_state(self.n, self.n_fft, self.hop, self.dev, prior=prior,
                                            out=self._state)
        if prior is not None:
            self._cur.copy_(prior[0])
        else:
            self._cur.zero_()
        self.samples_in = 0         # samples taken so far (per stream)
        self.frames_out = 0         # frames returned so far
        self._done = False

    def _advance(self, pcm, last):
        out, _ = ops.stft_stream_feed(self._state, pcm, self.samples_in, last, self.n_fft,
                                      self.hop, self._window, self.mode,
                                      fixed_offset=self._fixed, cur_offset=self._cur)
        self.samples_in += pcm.shape[1]
        self.frames_out += out.shape[2]
        return out.unsqueeze(1)

    def feed(self, pcm: torch.Tensor) -> torch.Tensor:
        """pcm [N, S], S >= 0, float32 or int16 on the device -> [N, 1, 161, k], k >= 0."""
        if self._done:
            raise RuntimeError("StreamingFrontend.feed after finish(): reset() starts an utterance")
        if not torch.is_tensor(pcm) or pcm.dim() != 2 or pcm.shape[0] != self.n:
            raise ValueError(f"pcm must be [{self.n}, S], got "
                             f"{tuple(pcm.shape) if torch.is_tensor(pcm) else type(pcm)}")
        if not pcm.is_cuda or pcm.dtype not in (torch.float32, torch.int16):
            raise ValueError("pcm must be a float32 or int16 device tensor")
        return self._advance(pcm.detach(), False)

    def finish(self) -> torch.Tensor:
        """The frames still held back, with the right reflection at the true end.  The
        utterance is closed afterwards (``reset`` starts the next)."""
        if self._done:
            raise RuntimeError("StreamingFrontend.finish called twice")
        self._done = True
        if self.samples_in == 0:
            return torch.empty(self.n, 1, ops.SPECT_ROWS, 0, device=self.dev, dtype=torch.float32)
        return self._advance(torch.empty(self.n, 0, device=self.dev, dtype=torch.float32), True)

    def offset(self) -> torch.Tensor:
        """float64 [N] on the device: the running mean S_t / (t + 1) of the frame means of
        'max_frame' (the prior's o0 before any frame; zeros for 'none')."""
        return self._cur.clone()


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


class StreamingTranscriber:
    """PCM chunks in, text out: ``StreamingFrontend`` -> ``StreamingSession`` -> a
    ``ds2amd.decoder.StreamingGreedyDecoder`` or ``StreamingBeamCTCDecoder``.

    ``t = StreamingTranscriber(model, decoder, n_streams=N)``; ``t.feed(pcm)`` with pcm [N, S] on
    the model's device returns what the decoder's ``feed`` returns for the output frames the
    chunk made final (the greedy decoder's delta, the beam decoder's current hypotheses);
    ``t.finish()`` flushes the front-end, then the session, and returns the decoder's ``feed`` of
    the last frames; ``t.text()`` is the decoder's.  audio_conf defaults to the model's;
    ``frontend_kw`` (normalize, offset, prior) go to the front-end.  One transcriber is one
    utterance per stream."""

    def __init__(self, model: dsm.DeepSpeech, decoder, audio_conf=None, n_streams: int = 1,
                 **frontend_kw):
        if not (hasattr(decoder, 'feed') and hasattr(decoder, 'text')):
            raise ValueError("StreamingTranscriber needs a streaming decoder "
                             "(StreamingGreedyDecoder or StreamingBeamCTCDecoder)")
        self.session = StreamingSession(model, n_streams=n_streams)
        if audio_conf is None:
            # the model's, with the defaults the model itself assumes for what it leaves out
            audio_conf = {'sample_rate': 16000, 'window_size': 0.02, 'window_stride': 0.01,
                          **model._audio_conf}
        self.frontend = StreamingFrontend(audio_conf, n_streams=n_streams,
                                          device=self.session.dev, **frontend_kw)
        self.decoder = decoder

    def feed(self, pcm: torch.Tensor):
        _, probs = self.session.feed(self.frontend.feed(pcm))
        return self.decoder.feed(probs)

    def finish(self):
        _, p1 = self.session.feed(self.frontend.finish())
        _, p2 = self.session.finish()
        return self.decoder.feed(torch.cat([p1, p2], 1))

    def text(self):
        return self.decoder.text()
