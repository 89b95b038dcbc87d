"""BSSSDR metric -- drop-in for the reference's ``fast_se_metrics.SDR`` (SDR.py:52-97), the BSS-eval
signal-to-distortion ratio with a 512-tap distortion filter (the quantity of
``torchmetrics.functional.audio.signal_distortion_ratio``).  The package's ``SDR`` class is another
metric (SI-SDR / SNR / SegSNR) and keeps its name; ``from fast_se_metrics.SDR import SDR`` is this one.

Rows are scored at 16 kHz (other rates go through BaseMetric's resampler, as for PESQ): both rows
are scaled to unit norm, the clean row's autocorrelation r and its cross-correlation b with the
denoised row are taken for the lags 0 ... 511, the Toeplitz system R x = b is solved, and the score
is ``10 log10(coh / (1 - coh))`` with ``coh = b . x`` (include/fsem_bsssdr.h).  ``use_gpu=True``: one
engine call (``fsem_bsssdr_f32``, csrc/bsssdr.hip, in libfsem_bsssdr.so); ``use_gpu=False``: the
package's CPU implementation (``_cpu.bsssdr``).  No warnings or exceptions for silent or empty rows:
a row whose system is singular (a silent clean row, a row of no samples) or that holds a non-finite
sample scores NaN, in that row only.

``differentiable_scores`` and ``loss`` are the same scores with the gradient with respect to the
denoised rows (include/fsem.h, "BSS-eval SDR with gradients"): on the engine
``fsem_bsssdr_state_f32`` forward, which keeps the solved filter of each row (4 KB), and
``fsem_bsssdr_grad_f32`` backward, one 512-tap pass in double (csrc/bsssdr_grad.hip, in libfsem.so); in
CPU mode ``_cpu.bsssdr64`` in float64 under torch's own autograd.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import (BaseMetric, check_row_rate, device_lengths, engine_rows, grad_buffer, grad_engine_rows,
                   grad_operands, noisy_shape, pair_rows, resample_rows, scored_mean)


class _EngineScores(torch.autograd.Function):
    """sdr [B] float32 of CUDA rows at rate ``sr`` by the engine, bitwise ``scores`` (fsem_bsssdr_state_f32,
    after the resampler for other rates), keeping the state; the backward is fsem_bsssdr_grad_f32 on that
    state and, for other rates, the transposed resampler (fsem_resample_rows_grad_f32) behind it: the
    gradient is taken at the float32 16 kHz rows the score was taken at.  ``clean`` and ``noisy`` are the rows
    as the engine reads them (float32, one stride, readable to ceil4(L)); the gradient comes back [B, width]."""

    @staticmethod
    def forward(ctx, noisy, clean, lens, L, sr, metric):
        B = clean.shape[0]
        ctx.shape, ctx.sr, ctx.lens = (B, L, noisy.shape[1]), sr, lens
        if sr != metric.EXPECTED_SAMPLING_RATE:  # (scores(): the forward resampler's float32 rows)
            clean, noisy, lens = resample_rows(clean[:, :L], noisy[:, :L], lens, sr, metric.EXPECTED_SAMPLING_RATE)
            clean, noisy, L, lens = engine_rows(*pair_rows(clean, noisy), lens)
        ctx.rows = (clean, noisy, lens, L)
        lib = _native.load()
        out = torch.empty(B, dtype=torch.float32, device=clean.device)
        ctx.state = torch.empty(lib.fsem_bsssdr_state_floats(B, L), dtype=torch.float32, device=clean.device)
        diag = 0.0 if metric.load_diag is None else float(metric.load_diag)
        rc = lib.fsem_bsssdr_state_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), _native.ptr(lens),
                                       diag, out.data_ptr(), ctx.state.data_ptr(),
                                       _native.stream_handle(clean.device))
        _native.check(rc, "BSSSDR")
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sdr):
        B = ctx.shape[0]
        clean, noisy, lens, L = ctx.rows
        at_rate = ctx.sr != 16000
        lib = _native.load()
        # (the 16 kHz gradient: the caller's buffer, or one as wide as the transposed resampler reads)
        shape16 = (B, L, max(L, int(lib.fsem_resample_length(ctx.shape[1], ctx.sr, 16000)))) if at_rate else ctx.shape
        grad, g = grad_buffer(shape16, B > 0, (g_sdr,))
        if g is None:
            return grad, None, None, None, None, None
        stream = _native.stream_handle(grad.device)
        rc = lib.fsem_bsssdr_grad_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), _native.ptr(lens),
                                      g[0].data_ptr(), ctx.state.data_ptr(), grad.data_ptr(), grad.stride(0), stream)
        _native.check(rc, "BSSSDR backward")
        if at_rate:
            grad16, (grad, _) = grad, grad_buffer(ctx.shape, True, (g_sdr,))
            rc = lib.fsem_resample_rows_grad_f32(grad16.data_ptr(), B, ctx.shape[1], grad16.stride(0),
                                                 _native.ptr(ctx.lens), grad.data_ptr(), grad.stride(0), ctx.sr, 16000,
                                                 stream)
            _native.check(rc, "BSSSDR backward")
        return grad, None, None, None, None, None


class BSSSDR(BaseMetric):
    higher_is_better = True
    EXPECTED_SAMPLING_RATE = 16000
    KEYS = ("SDR",)

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, devices=None):
        super().__init__(sample_rate, use_gpu, devices=devices)
        if use_gpu:
            _native.load_bsssdr()  # (a missing engine raises here, not at the first call)
        self.filter_length = 512
        self.zero_mean = False
        self.load_diag = None

    def scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, sample_rate: int | None = None,
               lengths=None) -> torch.Tensor:
        """sdr [B] float32 tensor (dB) on the metric's device, without a host sync.

        Rows at ``sample_rate``; None means rows already at 16 kHz, which requires a 16 kHz metric
        (``BSSSDR(8000).scores`` must be told its rows' rate).  Other rates are resampled to 16 kHz
        first, each row as the row alone.  ``lengths`` (optional, [B] ints at that rate): row b
        holds lengths[b] samples and scores as the unpadded row alone would.
        """
        sr = check_row_rate(self, sample_rate)
        if self.fans_out():
            if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
                raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
            return self.fan_out(lambda c, n, lk: self._rows_scores(c, n, sr, lk), clean_speech, denoised_speech,
                                lengths, 1, balance=lengths)[0]
        return self._rows_scores(clean_speech, denoised_speech, sr, lengths)

    def _rows_scores(self, clean_speech, denoised_speech, sr: int, lengths) -> torch.Tensor:
        """sdr [B] of rows at rate ``sr`` on their own device (one engine call)."""
        if self.zero_mean or self.filter_length != 512:
            raise NotImplementedError("BSSSDR: zero_mean = False and filter_length = 512 are fixed, as in the reference")
        if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        if sr != self.EXPECTED_SAMPLING_RATE:
            clean_speech, denoised_speech, lengths = resample_rows(clean_speech, denoised_speech, lengths, sr,
                                                                   self.EXPECTED_SAMPLING_RATE)
        clean, noisy = pair_rows(clean_speech, denoised_speech)
        B, L = clean.shape
        diag = self.load_diag
        if not clean.is_cuda:
            fn = _cpu.bsssdr if diag is None else (lambda c, n: _cpu.bsssdr(c, n, load_diag=diag))
            if lengths is not None:
                return _cpu.per_row(fn, clean, noisy, device_lengths(lengths, B, L, "cpu")).to(torch.float32)
            return _cpu.rows_parallel(fn, clean, noisy)
        lib = _native.load_bsssdr()
        # (the engine takes rows of at least one sample: a row of none is zero samples of length 0)
        clean, noisy, L, lens = engine_rows(clean, noisy, lengths, empty_as_zeros=True)
        out = torch.empty(B, dtype=torch.float32, device=clean.device)
        if B == 0:
            return out
        ws = _native.workspace(lib.fsem_bsssdr_workspace_bytes(B, L), clean.device)
        lp = _native.ptr(lens)
        if diag is None:
            rc = lib.fsem_bsssdr_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), lp, out.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _native.stream_handle(clean.device))
        else:
            rc = lib.fsem_bsssdr_load_diag_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0), lp,
                                               float(diag), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                               _native.stream_handle(clean.device))
        _native.check(rc, "BSSSDR")
        return out

    # ------------------------------------------------------------------ scores to train against
    def _differentiable(self, clean_speech, denoised_speech, sample_rate, lengths) -> torch.Tensor:
        """sdr [B] with the graph to ``denoised_speech`` (include/fsem.h, "BSS-eval SDR with gradients"):
        float32 from the engine on CUDA rows, float64 from ``_cpu.bsssdr64`` under torch's own autograd on host
        rows."""
        if self._fanout is not None:
            raise NotImplementedError("BSSSDR: devices= is not supported with gradients (the multi-device fan-out "
                                      "returns detached scores)")
        if self.zero_mean or self.filter_length != 512:
            raise NotImplementedError("BSSSDR: zero_mean = False and filter_length = 512 are fixed, as in the reference")
        sr = check_row_rate(self, sample_rate)
        clean, noisy = grad_operands(self, clean_speech, denoised_speech)
        if not clean.is_cuda:
            return self._differentiable_cpu(clean, noisy, sr, lengths)
        if clean.shape[1] == 0:  # rows of no samples: the scores, and an empty gradient
            return self._rows_scores(clean, noisy.detach(), sr, lengths) + noisy.to(torch.float32).sum(1) * 0
        clean, rows, L, lens = grad_engine_rows(clean, noisy, lengths)
        if clean.shape[0] == 0:
            return rows.sum(1) * 0
        return _EngineScores.apply(rows, clean, lens, L, sr, self)

    def _differentiable_cpu(self, clean, noisy, sr: int, lengths) -> torch.Tensor:
        B, L = clean.shape
        lens = device_lengths(lengths, B, L, "cpu").tolist() if lengths is not None else [L] * B
        out = []
        for b in range(B):  # (a plain loop: each row's graph hangs on its own slice of `noisy`)
            n = int(lens[b])
            c, row = clean[b:b + 1, :n], noisy[b:b + 1, :n]
            if sr != self.EXPECTED_SAMPLING_RATE and n > 0:
                # the value at the float32 rows scores() resamples, the derivative the resampler's in float64
                c, at, _ = resample_rows(c, row.detach(), None, sr, self.EXPECTED_SAMPLING_RATE)
                y = _cpu.resample64(row, sr, self.EXPECTED_SAMPLING_RATE)
                row = at.to(torch.float64) + (y - y.detach())
            out.append(_cpu.bsssdr64(c, row, self.load_diag))
        return torch.cat(out) if B else torch.zeros(0, dtype=torch.float64)

    def differentiable_scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor,
                              sample_rate: int | None = None, lengths=None) -> torch.Tensor:
        """sdr [B] (dB) as ``scores``, carrying the gradient with respect to ``denoised_speech``: float32 and
        bitwise ``scores()`` on the engine, float64 in CPU mode.  The clean rows are constants.  The gradient
        is taken at the float32 quotients h / |h| the score is taken at; a row that scores NaN gets a zero
        gradient row, and so does a row whose score sits at its floor of -80 dB (a silent estimate).  Rows at
        another rate are resampled as ``scores`` resamples them, to float32 16 kHz rows, and the gradient at
        those rows is pulled back through the transposed resampler (``fsem_resample_rows_grad_f32``).  LSD
        resamples in double there instead, to protect bins 100 dB below a frame's peak; SDR has no such
        bins: its correlations are sums over the whole row, which the rows' float32 rounding moves by 1e-7."""
        return self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)

    def loss(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, sample_rate: int | None = None,
             lengths=None) -> torch.Tensor:
        """-mean of SDR (higher is better) over the rows with a finite score: a scalar that carries the
        gradient with respect to ``denoised_speech``.  With no such row: a zero with a zero gradient."""
        sdr = self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)
        mean, _ = scored_mean(sdr, torch.isfinite(sdr.detach()), denoised_speech)
        return -mean

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            sdr = self.scores(clean_speech, denoised_speech, self.EXPECTED_SAMPLING_RATE, lengths=lengths)
            return self.result_list(sdr.float().reshape(1, -1))
