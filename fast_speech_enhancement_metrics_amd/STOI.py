"""STOI / ESTOI metric -- drop-in for the reference's ``fast_se_metrics.STOI`` (STOI.py:7-205).

Runs at 10 kHz internally (STOI.py:9).  ``use_gpu=True``: libfsem's gfx950 kernels
(``fsem_stoi_f32``) with the 16 -> 10 kHz resampler fused into them (the reference
resamples in BaseMetric.prepare_audio, base.py:19-20; same arithmetic), one device->host
copy of the scores.  ``use_gpu=False``: the package's CPU implementation.

``differentiable_scores`` and ``loss`` are the same scores with the gradient with respect to the
denoised rows (include/fsem.h, "STOI with gradients"): on the engine
``fsem_stoi_state_f32`` forward and ``fsem_stoi_grad_f32`` backward (csrc/stoi_grad.hip), in CPU mode
``_cpu.stoi`` in float64 under torch's own autograd.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _cpu, _native
from .base import (BaseMetric, check_row_rate, device_lengths, engine_rows, grad_buffer, grad_engine_rows,
                   grad_operands, noisy_shape, pair_rows, scored_mean, zero_tail)
from .batching import resampled_lengths

NO_SEGMENT = "Not enough non-silent frames. Please check your sound files"  # (the reference's warning, STOI.py:162-165)


def _bad_rate(sr: int) -> NotImplementedError:
    return NotImplementedError(f"unsupported sample rate {sr}: its resampling filter to 10 kHz would be longer "
                               "than 8192 taps (include/fsem.h, FSEM_ERATE)")


def _check(rc: int) -> None:
    if rc == _native.FSEM_ESHORT:
        raise RuntimeError("STOI input shorter than one 256-sample frame at 10 kHz")
    _native.check(rc, "STOI")


class _EngineScores(torch.autograd.Function):
    """(stoi, estoi [B] float32, segments [B] int32) of CUDA rows by the engine (fsem_stoi_state_f32, the
    kernels of fsem_stoi_f32 on a state of this call's own); the backward is fsem_stoi_grad_f32 on that
    state.  ``clean`` and ``noisy`` are the rows as the engine reads them (float32, one stride, readable
    to ceil4(L)); the gradient comes back [B, L]."""

    @staticmethod
    def forward(ctx, noisy, clean, lens, L, sr):
        lib = _native.load()
        B, dev = clean.shape[0], clean.device
        s = torch.empty(B, dtype=torch.float32, device=dev)
        e = torch.empty(B, dtype=torch.float32, device=dev)
        seg = torch.zeros(B, dtype=torch.int32, device=dev)
        ctx.mark_non_differentiable(seg)
        ctx.shape = (B, L, noisy.shape[1])
        ctx.state = None
        if B == 0:
            return s, e, seg
        nfloats = lib.fsem_stoi_state_floats(B, L, sr)
        if nfloats == 0:
            raise _bad_rate(sr)
        state = torch.empty(nfloats, dtype=torch.float32, device=dev)  # (not the shared workspace: it must outlive the call)
        _check(lib.fsem_stoi_state_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), _native.ptr(lens), sr,
                                       s.data_ptr(), e.data_ptr(), seg.data_ptr(), state.data_ptr(),
                                       _native.stream_handle(dev)))
        ctx.state, ctx.noisy, ctx.lens, ctx.sr = state, noisy, lens, sr
        return s, e, seg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_s, g_e, _g_seg):
        B, L, _ = ctx.shape
        grad, g = grad_buffer(ctx.shape, ctx.state is not None, (g_s, g_e))
        if g is None:
            return grad, None, None, None, None
        rc = _native.load().fsem_stoi_grad_f32(
            ctx.noisy.data_ptr(), B, L, ctx.noisy.stride(0), _native.ptr(ctx.lens), ctx.sr, ctx.state.data_ptr(),
            g[0].data_ptr(), g[1].data_ptr(), grad.data_ptr(), grad.stride(0), _native.stream_handle(grad.device))
        _native.check(rc, "STOI backward")
        return grad, None, None, None, None


class STOI(BaseMetric):
    higher_is_better = True
    EXPECTED_SAMPLING_RATE = 10000

    def __init__(self, sample_rate: int = 10000, use_gpu: bool = False, *, devices=None):
        super().__init__(sample_rate, use_gpu, devices=devices)
        self.sampling_frequency = self.EXPECTED_SAMPLING_RATE
        self.win_length = 256
        self.hop_length = self.win_length // 2
        self.n_fft = 512
        self.num_octave_bands = 15
        self.min_frequency = 150
        self.N = 30
        self.beta = -15.0
        self.dynamic_range = 40

    @staticmethod
    def normalize(x: torch.Tensor, dim: int = 0) -> torch.Tensor:
        """In place, as STOI.py:113-119: centre along ``dim`` and divide by the L2 norm, with the
        reference's ``1e-12 * randn`` term taken in expectation (deterministic, as the engine):
        the squared norm gains N * 1e-24 (N = x.shape[dim]) -- no change for any slice with a
        spread above ~1e-8, 0 for a zero-variance slice (the reference: a random unit vector),
        ~0 for a slice far below the noise.  Non-finite slices stay non-finite (NaN / Inf
        propagate as in the reference)."""
        x -= x.mean(dim=dim, keepdim=True)
        x /= torch.sqrt(x.square().sum(dim=dim, keepdim=True) + x.shape[dim] * 1e-24)
        return x

    # ------------------------------------------------------------------ reference attributes
    def get_octave_band_matrix(self) -> torch.Tensor:
        """[15, 257] float32 1/3-octave band matrix (STOI.py:26-47): band i covers the FFT bins
        from the one nearest 150 * 2^((2i - 1) / 6) Hz up to (excluding) the one nearest
        150 * 2^((2i + 1) / 6) Hz."""
        return _cpu._OBM.to(torch.float32).clone()

    @property
    def octave_band_matrix(self) -> torch.Tensor:
        """STOI.py:19, on the metric's device (built on first access)."""
        if getattr(self, "_octave_band_matrix", None) is None:
            self._octave_band_matrix = self.get_octave_band_matrix().to(self.device)
        return self._octave_band_matrix

    @property
    def window(self) -> torch.Tensor:
        """[256] float32 analysis window hann(257)[1:] (STOI.py:24), on the metric's device."""
        if getattr(self, "_window", None) is None:
            self._window = torch.hann_window(self.win_length + 1, dtype=torch.float32, device=self.device)[1:]
        return self._window

    # ------------------------------------------------------------------ stage methods
    # The reference's pipeline stages (STOI.py:49-198) on 10 kHz tensors, as torch expressions on
    # the metric's device (the overlap-add without the reference's per-utterance Python loop).
    # Scores do not go through these: on the GPU compute_metric runs the whole engine
    # (fsem_stoi_f32), which never materialises the overlap-added signal or the [B, S, 15, 30]
    # segments.
    def stft(self, speech: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """[N, T] -> [N, 257, frames] power spectrogram (n_fft 512, the 256-sample window centred,
        hop 128, center=False); frames at or past 1 + (length - 512) // 128 are zeroed (STOI.py:49-69)."""
        spec = torch.stft(speech, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                          window=self.window.to(speech.device, speech.dtype), center=False, normalized=False,
                          return_complex=True, onesided=True).abs().square()
        n_valid = 1 + (lengths.to(spec.device) - self.n_fft) // self.hop_length
        t = torch.arange(spec.shape[-1], device=spec.device)
        return spec.masked_fill((t[None, :] >= n_valid[:, None])[:, None, :], 0)

    def overlap_and_add(self, frames: torch.Tensor, lengths: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Kept frames [sum(lengths), 256] of B utterances (``lengths`` frames each, in order) ->
        (signals [B, max_len], (lengths + 1) * 128): frame j of utterance b added at 128 j
        (STOI.py:71-86)."""
        lengths = lengths.to(frames.device)
        out_len = (lengths + 1) * self.hop_length
        B = lengths.numel()
        width = int(out_len.max().item()) if B else 0
        sig = torch.zeros(B, width, dtype=frames.dtype, device=frames.device)
        if frames.numel():
            utt = torch.repeat_interleave(torch.arange(B, device=frames.device), lengths)
            first = torch.cumsum(lengths, 0) - lengths  # index of each utterance's first frame
            j = torch.arange(frames.shape[0], device=frames.device) - first[utt]
            pos = (utt * width + self.hop_length * j)[:, None] + torch.arange(self.win_length, device=frames.device)
            sig.view(-1).index_add_(0, pos.reshape(-1), frames.reshape(-1))
        return sig, out_len

    def remove_silent_frames(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor):
        """Frames (256, hop 128, windowed) more than 40 dB below the clean signal's loudest frame are
        dropped from both signals, which are rebuilt by overlap-add -> (clean, denoised, lengths)
        (STOI.py:88-111)."""
        w = self.window.to(clean_speech.device, clean_speech.dtype)
        cf = clean_speech.unfold(1, self.win_length, self.hop_length) * w
        df = denoised_speech.unfold(1, self.win_length, self.hop_length) * w
        energy = 20 * torch.log10(torch.linalg.vector_norm(cf, dim=2) + 1e-9)
        keep = (energy.amax(dim=1, keepdim=True) - self.dynamic_range - energy) < 0
        n = keep.sum(1)
        c, lens = self.overlap_and_add(cf[keep], n)
        d, _ = self.overlap_and_add(df[keep], n)
        return c, d, lens

    def compute_segments(self, speech: torch.Tensor, lengths: torch.Tensor):
        """1/3-octave band envelopes sqrt(OBM . |STFT|^2) [N, 15, T] cut into the T - 29 sliding
        30-frame windows (views) (STOI.py:121-127)."""
        obm = self.octave_band_matrix.to(speech.device, speech.dtype)
        tob = torch.sqrt(torch.matmul(obm, self.stft(speech, lengths)))
        return [tob[:, :, m:m + self.N] for m in range(max(tob.shape[2] - self.N + 1, 0))]

    def equalize_clip(self, clean_segments: torch.Tensor, denoised_segments: torch.Tensor) -> torch.Tensor:
        """Denoised segments scaled to the clean segments' norm over the 30 frames, then clipped at
        (1 + 10^(-beta/20)) x clean (STOI.py:129-139)."""
        nc = torch.linalg.vector_norm(clean_segments, dim=3, keepdim=True)
        nd = torch.linalg.vector_norm(denoised_segments, dim=3, keepdim=True)
        bound = clean_segments * (1 + 10 ** (-self.beta / 20))
        return torch.minimum(denoised_segments * (nc / (nd + 1e-9)), bound)

    def compute_correlation(self, clean_segments: torch.Tensor, denoised_segments: torch.Tensor,
                            mask: torch.Tensor, extended: bool) -> torch.Tensor:
        """Masked sum over (segment, band, frame) of the products, / 30 (ESTOI) or / 15 (STOI)
        (STOI.py:141-151)."""
        prod = denoised_segments * clean_segments * mask[:, :, None, None]
        return prod.sum(dim=(1, 2, 3)) / (self.N if extended else self.num_octave_bands)

    @torch.no_grad()
    def compute_stoi(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor):
        """(stoi [B], estoi [B]) of 10 kHz signals (STOI.py:153-198); with no 30-frame segment in
        the batch, the reference's warning and (tensor(0), tensor(0)).  GPU: the engine."""
        if clean_speech.is_cuda:
            s, e = self.scores(clean_speech, denoised_speech, self.EXPECTED_SAMPLING_RATE)
        else:
            s, e = _cpu.rows_parallel(_cpu.stoi, torch.atleast_2d(clean_speech), torch.atleast_2d(denoised_speech))
        if bool(torch.isnan(s).all()):
            warnings.warn(NO_SEGMENT, RuntimeWarning, stacklevel=2)
            return torch.tensor(0), torch.tensor(0)
        return s, e

    def scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, sample_rate: int | None = None,
               lengths=None):
        """(stoi[B], estoi[B]) tensors on the metric's device; NaN where no segment exists.

        Rows at ``sample_rate``; None means rows already at 10 kHz, which requires a 10 kHz metric
        (``STOI(16000).scores`` must be told its rows' rate).  ``lengths`` (optional, [B] ints at that rate):
        row b holds lengths[b] samples and scores as the reference would on the unpadded row.
        """
        sr = check_row_rate(self, sample_rate)
        if self.fans_out():
            if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
                raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
            return self.fan_out(lambda c, n, lk: self._rows_scores(c, n, sr, lk), clean_speech, denoised_speech,
                                lengths, 2, balance=lengths)
        return self._rows_scores(clean_speech, denoised_speech, sr, lengths)

    def _rows_scores(self, clean_speech, denoised_speech, sr: int, lengths):
        """(stoi [B], estoi [B]) of rows at rate ``sr`` on their own device (one engine call)."""
        clean, noisy = pair_rows(clean_speech, denoised_speech)
        B, L = clean.shape
        if not clean.is_cuda:
            clean, noisy = clean.detach(), noisy.detach()  # scores are detached, as the engine's (differentiable_scores)
            if lengths is not None:
                lens = device_lengths(lengths, B, L, "cpu")
                if sr != self.EXPECTED_SAMPLING_RATE:
                    clean, noisy = self._resample_cpu(zero_tail(clean, lens), sr), self._resample_cpu(zero_tail(noisy, lens), sr)
                    lens = resampled_lengths(lens, sr, self.EXPECTED_SAMPLING_RATE)
                return _cpu.per_row(_cpu.stoi, clean, noisy, lens)
            if sr != self.EXPECTED_SAMPLING_RATE:
                return _cpu.rows_parallel(lambda c, n: _cpu.stoi(self._resample_cpu(c, sr), self._resample_cpu(n, sr)),
                                          clean, noisy)
            return _cpu.rows_parallel(_cpu.stoi, clean, noisy)
        lib = _native.load()
        clean, noisy, L, lens = engine_rows(clean, noisy, lengths)
        s = torch.empty(B, dtype=torch.float32, device=clean.device)
        e = torch.empty(B, dtype=torch.float32, device=clean.device)
        nbytes = lib.fsem_stoi_workspace_bytes(B, L, sr)
        if nbytes == 0:
            raise _bad_rate(sr)
        ws = _native.workspace(nbytes, clean.device)
        _check(lib.fsem_stoi_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), _native.ptr(lens), sr,
                                 s.data_ptr(), e.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _native.stream_handle(clean.device)))
        return s, e

    # ------------------------------------------------------------------ scores to train against
    KEYS_LOSS = ("STOI", "ESTOI")

    def _differentiable(self, clean_speech, denoised_speech, sample_rate, lengths):
        """(stoi [B], estoi [B], segments [B]) with the graph to ``denoised_speech`` (include/fsem.h, "STOI with
        gradients"): float32 from the engine on CUDA rows, float64 from ``_cpu.stoi`` under torch's own
        autograd on host rows."""
        if self._fanout is not None:
            raise NotImplementedError("STOI: devices= is not supported with gradients (the multi-device fan-out "
                                      "returns detached scores)")
        sr = check_row_rate(self, sample_rate)
        clean, noisy = grad_operands(self, clean_speech, denoised_speech)
        if not clean.is_cuda:
            return self._differentiable_cpu(clean, noisy, sr, lengths)
        clean, rows, L, lens = grad_engine_rows(clean, noisy, lengths)
        return _EngineScores.apply(rows, clean, lens, L, sr)

    def _differentiable_cpu(self, clean, noisy, sr: int, lengths):
        B, L = clean.shape
        lens = device_lengths(lengths, B, L, "cpu").tolist() if lengths is not None else [L] * B
        nan = torch.full((1,), float("nan"), dtype=torch.float64)
        out_s, out_e, segs = [], [], []
        for b in range(B):  # (a plain loop: each row's graph hangs on its own slice of `noisy`)
            n = int(lens[b])
            c10 = _cpu.resample64(clean[b:b + 1, :n], sr, self.EXPECTED_SAMPLING_RATE)
            seg = int(_cpu.stoi_segments(c10)[0]) if c10.shape[1] >= 256 else 0
            segs.append(seg)
            row = noisy[b:b + 1, :n]
            if seg == 0:
                s, e = nan, nan
            elif not bool(torch.isfinite(row.detach()).all()):
                with torch.no_grad():  # a non-finite sample: the scores, no gradient (a zero row)
                    s, e = _cpu.stoi(c10, _cpu.resample64(row, sr, self.EXPECTED_SAMPLING_RATE))
            else:
                s, e = _cpu.stoi(c10, _cpu.resample64(row, sr, self.EXPECTED_SAMPLING_RATE))
            out_s.append(s)
            out_e.append(e)
        if not B:
            return torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.int32)
        return torch.cat(out_s), torch.cat(out_e), torch.tensor(segs, dtype=torch.int32)

    def differentiable_scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor,
                              sample_rate: int | None = None, lengths=None):
        """(stoi [B], estoi [B]) as ``scores``, carrying the gradient with respect to ``denoised_speech``:
        float32 and bitwise ``scores()`` on the engine (``fsem_stoi_state_f32`` / ``fsem_stoi_grad_f32``),
        float64 in CPU mode.  The clean rows are constants; a row without a segment (NaN) or with a
        non-finite sample gets a zero gradient; a zero band envelope takes the subgradient 0."""
        s, e, _ = self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)
        return s, e

    def loss(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, sample_rate: int | None = None,
             lengths=None, key: str = "ESTOI") -> torch.Tensor:
        """-mean of ``key`` ("STOI" or "ESTOI") over the rows that have a 30-frame segment: a scalar that
        carries the gradient with respect to ``denoised_speech``.  With no such row: the warning of the
        drop-in call and a zero with a zero gradient."""
        if key not in self.KEYS_LOSS:
            raise ValueError(f"key must be one of {list(self.KEYS_LOSS)}, not {key!r}")
        s, e, seg = self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)
        score = s if key == "STOI" else e
        mean, count = scored_mean(score, seg.to(score.device) > 0, denoised_speech)
        if count == 0:
            warnings.warn(NO_SEGMENT, RuntimeWarning, stacklevel=2)
            return mean
        return -mean

    def _finish(self, stois: torch.Tensor, estois: torch.Tensor) -> list[dict[str, float]]:
        t = torch.stack([stois.float(), estois.float()])
        if t.is_cuda:  # the dicts are built while the GPU computes, then filled
            res, host = _native.list_from_device(self, t, ("STOI", "ESTOI"))
            nan_all = bool(np.isnan(host[0]).all())
        else:
            res, nan_all = None, bool(torch.isnan(t[0]).all())
        if nan_all:  # no utterance has a 30-frame segment (STOI.py:162-165)
            warnings.warn(NO_SEGMENT, RuntimeWarning, stacklevel=3)
            raise TypeError("iteration over a 0-d tensor")
        return res if res is not None else _native.score_list(t, ("STOI", "ESTOI"))

    def _resample_cpu(self, x: torch.Tensor, sr: int) -> torch.Tensor:
        if sr == self.sample_rate:
            return self.resampler(x)
        from .resample import Resample
        return Resample(sr, self.EXPECTED_SAMPLING_RATE)(x)

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            return self._finish(*self.scores(clean_speech, denoised_speech, self.EXPECTED_SAMPLING_RATE,
                                             lengths=lengths))

    def __call__(self, clean_speech, denoised_speech, lengths=None) -> list[dict[str, float]]:
        if self.device == "cuda" and clean_speech is not None:
            # GPU: resampling is fused into the STOI kernels -- skip BaseMetric's resampler
            clean_speech, denoised_speech, lengths = self.split_ragged(clean_speech, denoised_speech, lengths)
            if clean_speech.shape != denoised_speech.shape:
                raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
            clean = torch.atleast_2d(clean_speech)
            noisy = torch.atleast_2d(denoised_speech)
            if not self.fans_out():  # (a multi-device metric's shards copy their own rows)
                clean, noisy = clean.to(self.home_device()), noisy.to(self.home_device())
            with torch.no_grad():
                return self._finish(*self.scores(clean, noisy, self.sample_rate, lengths=lengths))
        return super().__call__(clean_speech, denoised_speech, lengths)
