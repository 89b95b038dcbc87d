"""PESQ-wb metric -- drop-in for the reference's ``fast_se_metrics.PESQ`` (PESQ.py:13-245).

P.862-like wideband model without time alignment and with IIR level alignment
(reference PESQ.py:17-23).  ``use_gpu=True``: the whole per-utterance pipeline runs in
libfsem's gfx950 kernels (``fsem_pesq_wb_f32``) with one device->host copy of the scores;
``use_gpu=False``: the package's CPU implementation.

``differentiable_scores`` and ``loss`` are the same scores with the gradient with respect to the
denoised rows (include/fsem.h, "PESQ with gradients"): on the engine
``fsem_pesq_state_f32`` forward and ``fsem_pesq_grad_f32`` backward (csrc/pesq_grad.hip), in CPU mode
``_cpu.pesq_differentiable`` in float64 under torch's own autograd.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .bark import BarkFilterBank
from .base import (BaseMetric, as_rows, check_row_rate, device_lengths, engine_rows, grad_buffer, grad_engine_rows,
                   grad_operands, noisy_shape, pair_rows, resample_rows, same_device, scored_mean)
from .loudness import Loudness
from .spectrogram import Spectrogram


def _unit_rows(x: torch.Tensor, lengths=None) -> torch.Tensor:
    """Rows scaled by a power of two (exact) to a peak in [1, 2) of their first lengths[b] samples;
    zero / non-finite rows as they are."""
    a = x
    if lengths is not None:
        t = torch.arange(x.shape[1], device=x.device)
        a = x.masked_fill(t[None, :] >= torch.as_tensor(lengths, device=x.device).reshape(-1, 1), 0.0)
    peak = torch.linalg.vector_norm(a, ord=float("inf"), dim=1)  # max |x|: one pass over the rows
    ex = torch.where((peak > 0) & torch.isfinite(peak), torch.floor(torch.log2(peak)), torch.zeros_like(peak))
    return x * torch.exp2(-ex).to(x.dtype)[:, None]  # a power of two: exact, as ldexp


def _too_short(F: int) -> RuntimeError:
    """The reference's unfold(1, size=20, step=10) fails on fewer than 20 frames (PESQ.py:169)."""
    return RuntimeError(f"maximum size for tensor at dimension 1 is {max(F, 0)} but size is 20")


def _wb_frames(lib, clean: torch.Tensor, noisy: torch.Tensor, lens):
    """(distances [2, B], per-frame disturbances [B, 2, F]) of 16 kHz rows on the GPU through the
    whole-metric entry (fsem_pesq_wb_frames_f32: its range handling, no host-side row scaling)."""
    # (this path hands the entry rows that lie back to back: views with a longer row stride are copied)
    clean, noisy = as_rows(clean).contiguous(), as_rows(noisy).contiguous()
    B, L = clean.shape
    F = lib.fsem_pesq_frames(L)
    if F < 20 and lens is None:
        raise _too_short(F)
    clean, noisy, L, lens = engine_rows(clean, noisy, lens)
    mos = torch.empty(B, dtype=torch.float32, device=clean.device)
    dist = torch.empty(2, B, dtype=torch.float32, device=clean.device)
    frames = torch.full((B, 2, F), float("nan"), device=clean.device)
    ws = _native.workspace(lib.fsem_pesq_workspace_bytes(B, L), clean.device)
    _native.check(lib.fsem_pesq_wb_frames_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0),
                                              _native.ptr(lens), mos.data_ptr(), dist.data_ptr(), frames.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _native.stream_handle(clean.device)),
                  "PESQ frames")
    return dist[0], frames


class _EngineScores(torch.autograd.Function):
    """(mos, symmetric distance, asymmetric distance [B] float32) of 16 kHz CUDA rows by the engine
    (fsem_pesq_state_f32, the kernels of fsem_pesq_wb_frames_f32 on a state of this call's own); the
    backward is fsem_pesq_grad_f32 on that state.  ``clean`` and ``noisy`` are the rows as the engine
    reads them (float32, one stride, readable to ceil4(L)); the gradient comes back [B, width]."""

    @staticmethod
    def forward(ctx, noisy, clean, lens, L):
        lib = _native.load()
        B, dev = clean.shape[0], clean.device
        mos = torch.empty(B, dtype=torch.float32, device=dev)
        dist = torch.empty(2, B, dtype=torch.float32, device=dev)
        ctx.shape = (B, L, noisy.shape[1])
        ctx.state = None
        if B == 0:
            return mos, dist[0], dist[1]
        state = torch.empty(lib.fsem_pesq_state_floats(B, L), dtype=torch.float32, device=dev)  # (outlives the call)
        rc = lib.fsem_pesq_state_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), _native.ptr(lens),
                                     mos.data_ptr(), dist.data_ptr(), state.data_ptr(), _native.stream_handle(dev))
        if rc == _native.FSEM_ESHORT:
            raise _too_short(lib.fsem_pesq_frames(L))
        _native.check(rc, "PESQ")
        ctx.state, ctx.noisy, ctx.lens = state, noisy, lens
        return mos, dist[0], dist[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mos, g_sym, g_asym):
        B, L, _ = ctx.shape
        grad, g = grad_buffer(ctx.shape, ctx.state is not None, (g_mos, g_sym, g_asym))
        if g is None:
            return grad, None, None, None
        rc = _native.load().fsem_pesq_grad_f32(
            ctx.noisy.data_ptr(), B, L, ctx.noisy.stride(0), _native.ptr(ctx.lens), ctx.state.data_ptr(),
            g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), grad.data_ptr(), grad.stride(0),
            _native.stream_handle(grad.device))
        _native.check(rc, "PESQ backward")
        return grad, None, None, None


class PESQ(BaseMetric):
    higher_is_better = True
    EXPECTED_SAMPLING_RATE = 16000

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, time_align=False,
                 max_delay: int = 16000, devices=None):
        """``time_align`` (extension, off by default as in the reference, PESQ.py:19-22): shift each
        degraded row by its estimated delay before scoring (``alignment.time_align``, P.862-style;
        ``max_delay`` samples at 16 kHz bounds the search): True or "row" -- one delay per row;
        "utterance" -- P.862's per-utterance delays, the row realigned segment by segment;
        "p862" -- the same with P.862's histogram fine stage and recursive utterance split.  The
        delays of the last scored batch (per row; in the segment modes each row's longest
        segment's) are kept in ``last_delays``.  ``devices``: see BaseMetric (multi-device calls)."""
        super().__init__(sample_rate, use_gpu, devices=devices)
        if time_align not in (False, True, "row", "utterance", "p862"):
            raise ValueError('time_align must be False, True, "row", "utterance" or "p862"')
        self.time_align = "row" if time_align is True else time_align
        self.max_delay = int(max_delay)
        self.last_delays = None

    @staticmethod
    def equalize_ranges(clean_speech: torch.Tensor, noisy_speech: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Both rows divided by their joint peak |x| (PESQ.py:115-121).  The engine skips this step:
        it cancels under the level alignment (amplitude range)."""
        m = torch.maximum(clean_speech.abs().amax(dim=1, keepdim=True), noisy_speech.abs().amax(dim=1, keepdim=True))
        return clean_speech / m, noisy_speech / m

    # ------------------------------------------------------------------ reference attributes
    # The reference's constructor attributes (PESQ.py:63-90), on the metric's device, built on
    # first access (the engine carries its own copies in constant memory).
    @property
    def power_filter(self) -> torch.Tensor:
        """[2, 11] (b; a) of the order-5 Butterworth band-pass 325-3250 Hz at 16 kHz (PESQ.py:80-81)."""
        if getattr(self, "_power_filter", None) is None:
            import numpy as np
            from scipy.signal import butter
            out = np.asarray(butter(5, [325, 3250], fs=16000, btype="band"))
            self._power_filter = torch.as_tensor(out, device=self.device, dtype=torch.float32)
        return self._power_filter

    @property
    def pre_filter(self) -> torch.Tensor:
        """[2, 3] (b; a) of the pre-emphasis IIR (PESQ.py:84-88)."""
        if getattr(self, "_pre_filter", None) is None:
            self._pre_filter = torch.tensor([[2.740826, -5.4816519, 2.740826], [1.0, -1.9444777, 0.94597794]],
                                            device=self.device, dtype=torch.float32)
        return self._pre_filter

    @property
    def taper_weights(self) -> torch.Tensor:
        """[15] edge taper (k + 1) / 16 of the first / last 15 samples (PESQ.py:90)."""
        if getattr(self, "_taper_weights", None) is None:
            self._taper_weights = torch.linspace(0, 15, 16, device=self.device)[1:] / 16.0
        return self._taper_weights

    @property
    def to_spec(self) -> Spectrogram:
        """Hann-512 / hop-256 power spectrogram, center=False (PESQ.py:63-71)."""
        if getattr(self, "_to_spec", None) is None:
            self._to_spec = Spectrogram(win_length=512, n_fft=512, hop_length=256, window_fn=torch.hann_window,
                                        power=2, normalized=False, center=False).to(self.device)
        return self._to_spec

    @property
    def filter_bank(self) -> BarkFilterBank:
        """P.862 Bark filterbank, 256 bins -> 49 bands (PESQ.py:74)."""
        if getattr(self, "_filter_bank", None) is None:
            self._filter_bank = BarkFilterBank(256, 49, device=self.device)
        return self._filter_bank

    @property
    def loudness(self) -> Loudness:
        """Zwicker loudness model over the 49 bands (PESQ.py:77)."""
        if getattr(self, "_loudness", None) is None:
            self._loudness = Loudness(49, device=self.device)
        return self._loudness

    # ------------------------------------------------------------------ stage methods
    # The reference's pipeline stages (PESQ.py:92-230) on [rows, samples] tensors of 16 kHz
    # speech.  On the GPU the band-pass power and the Bark bands come from the engine's front end
    # (fsem_pesq_front_f32) and the disturbances from its back end (fsem_pesq_distances_f32); the
    # remaining stages are short torch expressions on the metric's device.  Scores do not go
    # through these methods: compute_metric runs the whole engine in one call.
    def _front(self, speech: torch.Tensor):
        """Engine front end on any number of rows -> (unscaled Bark bands [N, F, 49], sum of the
        squared band-pass output [N]), float64.  Rows go in scaled by a power of two to a peak
        in [1, 2) (exact) and the results come back at the rows' own scale in float64, so the
        float32 stage outputs cannot overflow for any finite input."""
        x = as_rows(speech)
        N, L = x.shape
        peak = x.abs().amax(dim=1)
        ex = torch.where((peak > 0) & torch.isfinite(peak), torch.floor(torch.log2(peak)), torch.zeros_like(peak))
        x = _unit_rows(x).contiguous()
        if L % 4 or N % 2:
            x = torch.nn.functional.pad(x, (0, (-L) % 4))
            if N % 2:
                x = torch.cat([x, x[-1:]], 0)  # the front end takes rows in (ref, deg) halves
            x = x.contiguous()
        h = x.shape[0] // 2
        lib = _native.load()
        F = lib.fsem_pesq_frames(L)
        if F < 1:
            raise RuntimeError("PESQ input shorter than one 512-sample frame")
        fld = (F + 31) // 32 * 32
        bark = torch.empty(2 * h, 49, fld, device=x.device)
        power = torch.empty(2 * h, device=x.device)
        ws = _native.workspace(lib.fsem_pesq_front_workspace_bytes(h, L), x.device)
        _native.check(lib.fsem_pesq_front_f32(x[:h].data_ptr(), x[h:].data_ptr(), h, L, x.stride(0), None,
                                              bark.data_ptr(), power.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _native.stream_handle(x.device)), "PESQ front")
        g = torch.exp2(2 * ex.double())
        return bark[:N, :, :F].transpose(1, 2).double() * g[:, None, None], power[:N].double() * g

    def align_level(self, speech: torch.Tensor) -> torch.Tensor:
        """Rows scaled to band-pass power 1e7 (PESQ.py:92-102): x * sqrt(1e7 / P) with
        P = sum(bandpass(x)^2) / (L + 5120) / 1.04684."""
        speech = torch.atleast_2d(speech)
        L = speech.shape[1]
        if speech.is_cuda and _cpu.pesq_frames(L) >= 1:
            p = self._front(speech)[1]
        else:
            # host float64 cascade: CPU rows, and rows shorter than one 512-sample frame (the
            # engine's front end frames what it filters; the reference filters any length)
            p = torch.from_numpy(_cpu.bandpass_power(speech.detach().to("cpu", torch.float64).numpy()))
        gain = _cpu.level_scale(p, L).sqrt().to(speech.device, speech.dtype)
        return speech * gain[:, None]

    def pre_emphasize(self, speech: torch.Tensor) -> torch.Tensor:
        """Edge taper (in place on ``speech``, as the reference) and the pre-emphasis IIR
        (PESQ.py:104-113); float32 rows stay float32, on the GPU the filter runs on the device
        (fsem_pre_emphasize_f32, torchaudio's float32 evaluation order)."""
        w = self.taper_weights.to(speech.device, speech.dtype)
        speech[:, :15] *= w
        speech[:, -15:] *= torch.flip(w, dims=(0,))
        if speech.is_cuda:
            x = as_rows(speech)
            y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            lib = _native.load()
            _native.check(lib.fsem_pre_emphasize_f32(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), y.data_ptr(),
                                                     y.stride(0), _native.stream_handle(x.device)), "pre-emphasis")
            return y.to(speech.dtype)
        from scipy.signal import lfilter
        y = lfilter(_cpu._PRE_B, _cpu._PRE_A, speech.detach().to("cpu", torch.float64).numpy(), axis=1)
        return torch.from_numpy(y).to(speech.device, speech.dtype)

    def get_bark_bands(self, speech: torch.Tensor) -> torch.Tensor:
        """[N, L] rows -> [N, F, 49] float64 Bark power bands after level alignment and
        pre-emphasis (PESQ.py:123-140)."""
        speech = torch.atleast_2d(speech)
        if not speech.is_cuda:
            return _cpu.bark_of_rows(speech).to(speech.device)
        bark, p = self._front(speech)
        return bark * _cpu.level_scale(p, speech.shape[1])[:, None, None]

    def equalize_bark_bands(self, clean_bark_bands: torch.Tensor, noisy_bark_bands: torch.Tensor):
        """(clean, noisy) Bark bands after the band and frame power equalisation (PESQ.py:142-166)."""
        return _cpu.equalize(clean_bark_bands, noisy_bark_bands)

    def get_overlapping_sums(self, disturbance: torch.Tensor) -> torch.Tensor:
        """[B, F] -> [B]: L6 over 20-frame windows (hop 10), then L2 over windows (PESQ.py:168-172)."""
        return _cpu.overlapping_sums(disturbance)

    def get_disturbances(self, clean_speech: torch.Tensor, noisy_speech: torch.Tensor):
        """(symmetric, asymmetric) distances [B] of 16 kHz pairs (PESQ.py:174-230); MOS =
        0.999 + 4 / (1 + exp(-1.3669 (4.5 - 0.1 sym - 0.0309 asym) + 3.8224))."""
        clean = as_rows(clean_speech)
        noisy = as_rows(noisy_speech)
        if clean.shape != noisy.shape:
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        if not clean.is_cuda:
            return _cpu.pesq_distances(clean, noisy)
        sym, asym, _ = self.frame_disturbances(clean, noisy)
        return sym, asym

    def frame_disturbances(self, clean_speech: torch.Tensor, noisy_speech: torch.Tensor, lengths=None):
        """Engine back-end intermediates of 16 kHz pairs: (symmetric distance [B], asymmetric
        distance [B], per-frame disturbances [B, 2, F] -- symmetric then asymmetric, after the
        frame weighting and the clamp at 45, PESQ.py:222-224).  GPU only (the stage entry
        fsem_pesq_distances_f32); rows under 20 frames give NaN distances."""
        # each signal is level-aligned on its own (PESQ.py:92-102), so scaling a row by a power of
        # two changes nothing but the range: rows go in with peaks in [1, 2), as _front
        clean, noisy = as_rows(clean_speech), as_rows(noisy_speech)
        same_device(clean, noisy)
        lib = _native.load()
        B = clean.shape[0]
        clean, noisy, L, lens = engine_rows(_unit_rows(clean, lengths), _unit_rows(noisy, lengths), lengths)
        F = lib.fsem_pesq_frames(L)
        if F < 20 and lens is None:
            raise _too_short(F)
        fld = (F + 31) // 32 * 32
        bark = torch.empty(2 * B, 49, fld, device=clean.device)
        power = torch.empty(2 * B, device=clean.device)
        st = _native.stream_handle(clean.device)
        ws = _native.workspace(max(lib.fsem_pesq_front_workspace_bytes(B, L),
                                   lib.fsem_pesq_distances_workspace_bytes(B, L)), clean.device)
        lp = _native.ptr(lens)
        _native.check(lib.fsem_pesq_front_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), lp,
                                              bark.data_ptr(), power.data_ptr(), ws.data_ptr(), ws.numel(), st),
                      "PESQ front")
        dist = torch.empty(2, B, device=clean.device)
        frames = torch.full((B, 2, F), float("nan"), device=clean.device)
        _native.check(lib.fsem_pesq_distances_f32(bark.data_ptr(), power.data_ptr(), B, L, lp, dist.data_ptr(),
                                                  frames.data_ptr(), ws.data_ptr(), ws.numel(), st),
                      "PESQ distances")
        return dist[0], dist[1], frames

    # ------------------------------------------------------------------ device paths
    def scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, lengths=None,
               sample_rate: int | None = None) -> torch.Tensor:
        """Per-utterance MOS as a tensor on the metric's device (no host sync on GPU).

        Rows at ``sample_rate``; None means rows already at 16 kHz, which requires a 16 kHz metric
        (a ``PESQ(8000)`` must be told its rows' rate, or it would score them as 16 kHz).  Other
        rates are resampled to 16 kHz first, each row as the row alone (BaseMetric.prepare_audio,
        base.py:19-20).  ``lengths`` (optional, [B] ints at that rate): row b holds lengths[b]
        samples and scores as the reference would on that unpadded row alone; rows under 20
        frames give NaN.
        """
        sr = check_row_rate(self, sample_rate)
        if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        if isinstance(clean_speech, torch.Tensor):  # scores are detached (differentiable_scores carries the graph)
            clean_speech = clean_speech.detach()
        if isinstance(denoised_speech, torch.Tensor):
            denoised_speech = denoised_speech.detach()
        aligned = getattr(self, "time_align", False)
        if self.fans_out():
            def shard(c, n, lk):
                mos, delays = self._rows_scores(c, n, lk, sr)
                return (mos, delays.to(torch.int32)) if aligned else mos  # FanOut keeps the dtype: exact delays

            cols = self.fan_out(shard, clean_speech, denoised_speech, lengths, 2 if aligned else 1, balance=lengths)
            if aligned:
                self.last_delays = cols[1].to(torch.int32)
            return cols[0]
        mos, delays = self._rows_scores(clean_speech, denoised_speech, lengths, sr)
        if aligned:
            self.last_delays = delays
        return mos

    def _rows_scores(self, clean_speech, denoised_speech, lengths, sr: int):
        """(mos [B], delays [B] or None) of rows at rate ``sr`` on their own device (one engine call)."""
        delays = None
        if sr != self.EXPECTED_SAMPLING_RATE:
            clean_speech, denoised_speech, lengths = resample_rows(clean_speech, denoised_speech, lengths, sr,
                                                                   self.EXPECTED_SAMPLING_RATE)
        clean, noisy = pair_rows(clean_speech, denoised_speech)
        B, L = clean.shape
        if getattr(self, "time_align", False) == "p862":
            mos, delays, _, _ = self.p862_scores(clean, noisy, lengths)
            return mos, delays
        if getattr(self, "time_align", False):
            from .alignment import time_align
            noisy, delays = time_align(clean, noisy, lengths, self.max_delay, mode=self.time_align)
        lib = _native.load() if clean.is_cuda else None
        if lib is None:
            if lengths is None:
                return _cpu.rows_parallel(_cpu.pesq, clean, noisy), delays
            return _cpu.per_row(_cpu.pesq, clean, noisy, device_lengths(lengths, B, L, "cpu")), delays
        clean, noisy, L, lens = engine_rows(clean, noisy, lengths)
        F = lib.fsem_pesq_frames(L)
        if F < 20 and lens is None:
            raise _too_short(F)
        mos = torch.empty(B, dtype=torch.float32, device=clean.device)
        ws = _native.workspace(lib.fsem_pesq_workspace_bytes(B, L), clean.device)
        _native.check(lib.fsem_pesq_wb_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), _native.ptr(lens),
                                           mos.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _native.stream_handle(clean.device)), "PESQ")
        return mos, delays

    # ------------------------------------------------------------------ scores to train against
    KEYS_LOSS = ("PESQ", "distance")

    def _differentiable(self, clean_speech, denoised_speech, sample_rate, lengths):
        """(mos [B], symmetric distance [B], asymmetric distance [B], scored [B] bool) with the graph to
        ``denoised_speech`` (include/fsem.h, "PESQ with gradients"): float32 from the engine on CUDA rows,
        float64 from ``_cpu.pesq_differentiable`` under torch's own autograd on host rows.  ``scored``: the
        row has at least 20 frames."""
        if self._fanout is not None:
            raise NotImplementedError("PESQ: devices= is not supported with gradients (the multi-device fan-out "
                                      "returns detached scores): use one device per process")
        if getattr(self, "time_align", False):
            raise NotImplementedError("PESQ: time_align is not supported with gradients (the delay search is not "
                                      "differentiable): align the rows first (alignment.time_align) and use "
                                      "PESQ(time_align=False)")
        sr = check_row_rate(self, sample_rate)
        clean, noisy = grad_operands(self, clean_speech, denoised_speech)
        if not clean.is_cuda:
            return self._differentiable_cpu(clean, noisy, sr, lengths)
        if sr != self.EXPECTED_SAMPLING_RATE:
            raise NotImplementedError(f"PESQ: the engine's gradients take rows at 16 kHz, not {sr} Hz: resample the "
                                      "rows first with differentiable torch ops, or use PESQ(use_gpu=False)")
        clean, rows, L, lens = grad_engine_rows(clean, noisy, lengths)
        F = _native.load().fsem_pesq_frames(L)
        if F < 20 and lens is None:
            raise _too_short(F)
        mos, sym, asym = _EngineScores.apply(rows, clean, lens, L)
        if lens is None:
            scored = torch.ones(clean.shape[0], dtype=torch.bool, device=clean.device)
        else:
            n = lens.to(torch.int64)
            scored = (n + n % 256) >= 512 + 19 * 256
        return mos, sym, asym, scored

    def _differentiable_cpu(self, clean, noisy, sr: int, lengths):
        B, L = clean.shape
        lens = device_lengths(lengths, B, L, "cpu").tolist() if lengths is not None else [L] * B
        rate = self.EXPECTED_SAMPLING_RATE
        if lengths is None and B:
            F = _cpu.pesq_frames(_cpu.resample64(clean[:1], sr, rate).shape[1])
            if F < 20:  # as scores()
                raise _too_short(F)
        nan = torch.full((1,), float("nan"), dtype=torch.float64)
        outs, scored = [], []
        for b in range(B):  # (a plain loop: each row's graph hangs on its own slice of `noisy`)
            n = int(lens[b])
            c16 = _cpu.resample64(clean[b:b + 1, :n], sr, rate)
            ok = _cpu.pesq_frames(c16.shape[1]) >= 20
            scored.append(ok)
            row = noisy[b:b + 1, :n]
            if not ok:
                outs.append((nan, nan, nan))
                continue
            out = _cpu.pesq_differentiable(c16, _cpu.resample64(row, sr, rate))
            if not bool(torch.isfinite(out[0].detach()).all()):
                # zero band-pass power or a non-finite sample: the scores, no gradient (a zero row)
                out = tuple(o.detach() for o in out)
            outs.append(out)
        if not B:
            z = torch.zeros(0, dtype=torch.float64)
            return z, z.clone(), z.clone(), torch.zeros(0, dtype=torch.bool)
        return (*(torch.cat([o[i] for o in outs]) for i in range(3)), torch.tensor(scored))

    def differentiable_scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor,
                              sample_rate: int | None = None, lengths=None) -> torch.Tensor:
        """MOS [B] as ``scores``, carrying the gradient with respect to ``denoised_speech``: float32 and
        bitwise ``scores()`` on the engine (``fsem_pesq_state_f32`` / ``fsem_pesq_grad_f32``, rows at 16 kHz),
        float64 in CPU mode (any rate ``scores`` takes).  The clean rows are constants; a row under 20
        frames (NaN), with a non-finite score or sample, or on the engine's range path gets a zero gradient."""
        return self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)[0]

    def loss(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, sample_rate: int | None = None,
             lengths=None, key: str = "PESQ") -> torch.Tensor:
        """A scalar that carries the gradient with respect to ``denoised_speech``, over the rows that have
        at least 20 frames: ``key="PESQ"`` -mean MOS; ``key="distance"`` +mean of 0.1 d_sym + 0.0309 d_asym,
        the quantity under the MOS mapping's sigmoid, which does not saturate at either end of the scale.
        With no such row: a zero with a zero gradient."""
        if key not in self.KEYS_LOSS:
            raise ValueError(f"key must be one of {list(self.KEYS_LOSS)}, not {key!r}")
        mos, sym, asym, scored = self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)
        score = -mos if key == "PESQ" else 0.1 * sym + 0.0309 * asym
        return scored_mean(score, scored, denoised_speech)[0]

    def p862_scores(self, clean_speech: torch.Tensor, noisy_speech: torch.Tensor, lengths=None):
        """The ``time_align="p862"`` scores of 16 kHz rows (extension, not in the reference,
        PESQ.py:19-22): the P.862-mode alignment (``alignment.time_align_segments``), the aligned
        rows' per-frame disturbances, P.862's realignment of bad intervals
        (``alignment.realign_bad_intervals``), the realigned rows' disturbances (only rows with an
        interval), and the MOS of the frames each interval scores better with
        (``fsem_pesq_pool_f32``).  Returns (mos [B] float32, delays [B], n_bad [B], bad [B, 16, 3])
        on the rows' device (CPU rows: _cpu.pesq_p862, mos float64)."""
        from . import alignment
        clean = as_rows(clean_speech)
        noisy = as_rows(noisy_speech)
        same_device(clean, noisy)
        B, L = clean.shape
        max_delay = getattr(self, "max_delay", alignment.DEFAULT_MAX_DELAY)
        if not clean.is_cuda:
            lens = None if lengths is None else device_lengths(lengths, B, L, "cpu")
            return _cpu.pesq_p862(clean, noisy, lens, max_delay)
        lib = _native.load()
        lens = device_lengths(lengths, B, L, clean.device) if lengths is not None else None
        aligned, delays, nseg, starts, sdel = alignment.time_align_segments(clean, noisy, lens, max_delay, mode="p862")
        ds, fr1 = _wb_frames(lib, clean, aligned, lens)
        n_bad, bad, second = alignment.realign_bad_intervals(clean, noisy, aligned, fr1, nseg, starts, sdel, lens)
        fr2 = fr1
        rows = torch.nonzero(n_bad).flatten()  # host sync: the second scoring covers these rows only
        if 2 * rows.numel() > B:
            # most rows: score the whole batch again rather than gather them (a row without an
            # interval has second == aligned, so its frames come out as fr1's)
            _, fr2 = _wb_frames(lib, clean, second, lens)
        elif rows.numel():
            fr2 = fr1.clone()
            _, sub = _wb_frames(lib, clean[rows], second[rows], None if lens is None else lens[rows])
            fr2[rows] = sub
        mos = torch.empty(B, dtype=torch.float32, device=clean.device)
        _native.check(lib.fsem_pesq_pool_f32(fr1.data_ptr(), fr2.data_ptr(), ds.data_ptr(), B, L, _native.ptr(lens),
                                             n_bad.data_ptr(), bad.data_ptr(), mos.data_ptr(),
                                             _native.stream_handle(clean.device)), "PESQ pool")
        return mos, delays, n_bad, bad

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.inference_mode():
            mos = self.scores(clean_speech, denoised_speech, lengths, sample_rate=self.EXPECTED_SAMPLING_RATE)
            if not mos.is_cuda:
                return _native.score_list(mos.reshape(1, -1), ("PESQ",))
            return _native.list_from_device(self, mos.reshape(1, -1), ("PESQ",))[0]
