"""LSD metric -- drop-in for the reference's ``fast_se_metrics.LSD`` (LSD.py:6-52), the
log-spectral distance of the URGENT challenge's evaluation.

Rows are scored at 16 kHz (other rates go through BaseMetric's resampler, as for PESQ): the
denoised row is scaled onto the clean one, both get a centred 512-point STFT (hop 256, periodic
Hann window), and the score is the mean over frames of the root mean square over the 257 bins of
``ln(S^2 / (H + 1e-8)^2 + 1e-8)`` (include/fsem_lsd.h).  ``use_gpu=True``: one engine call
(``fsem_lsd_f32``, csrc/lsd.hip, in libfsem_lsd.so); ``use_gpu=False``: the package's CPU
implementation (``_cpu.lsd``).  No warnings or exceptions for silent or empty rows: they score as
the definition says (ln 1e8 = 18.42068 for a silent clean row or a row of no samples).

``differentiable_scores`` and ``loss`` are the same scores with the gradient with respect to the
denoised rows (include/fsem.h, "LSD with gradients"): on the engine
``fsem_lsd_f32`` forward and ``fsem_lsd_grad_f32`` backward (csrc/lsd_grad.hip, in libfsem.so), which
keeps nothing of the forward; in CPU mode ``_cpu.lsd64`` in float64 under torch's own autograd.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import (BaseMetric, check_row_rate, device_lengths, engine_rows, grad_buffer, grad_engine_rows,
                   grad_operands, noisy_shape, pair_rows, resample_rows, scored_mean)


def _engine_scores(clean: torch.Tensor, noisy: torch.Tensor, B: int, L: int, lens) -> torch.Tensor:
    """lsd [B] float32 of engine_rows' CUDA rows: one fsem_lsd_f32 call."""
    lib = _native.load_lsd()
    out = torch.empty(B, dtype=torch.float32, device=clean.device)
    if B == 0:
        return out
    ws = _native.workspace(lib.fsem_lsd_workspace_bytes(B, L), clean.device)
    rc = lib.fsem_lsd_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0),
                          _native.ptr(lens), out.data_ptr(), ws.data_ptr(),
                          ws.numel(), _native.stream_handle(clean.device))
    _native.check(rc, "LSD")
    return out


class _EngineScores(torch.autograd.Function):
    """lsd [B] float32 of CUDA rows at rate ``sr`` by the engine, as ``scores`` (fsem_lsd_f32, after the
    resampler for other rates).  The backward is fsem_lsd_grad_rate_f32 (at 16 kHz: fsem_lsd_grad_f32) on
    the same rows and a scratch state of its own: the forward keeps nothing but the operands.  At other
    rates that entry differentiates LSD at the rows resampled in DOUBLE, not at the float32 rows the score
    was taken at (a deliberate departure: include/fsem.h, INTEGRATION.md section 18, Precision).
    ``clean`` and ``noisy`` are the rows as the engine reads them (float32, one stride, readable to
    ceil4(L)); the gradient comes back [B, L]."""

    @staticmethod
    def forward(ctx, noisy, clean, lens, L, sr, metric):
        B = clean.shape[0]
        ctx.shape = (B, L, noisy.shape[1])
        ctx.noisy, ctx.clean, ctx.lens, ctx.sr = noisy, clean, lens, sr
        if sr != metric.EXPECTED_SAMPLING_RATE:  # (scores(): the forward resampler's float32 rows)
            return metric._rows_scores(clean[:, :L], noisy[:, :L], sr, lens)
        return _engine_scores(clean, noisy, B, L, lens)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_lsd):
        B, L, _ = ctx.shape
        grad, g = grad_buffer(ctx.shape, B > 0, (g_lsd,))
        if g is None:
            return grad, None, None, None, None, None
        lib = _native.load()
        nfloats = lib.fsem_lsd_grad_rate_state_floats(B, L, ctx.sr)
        if nfloats == 0:
            _native.check(_native.FSEM_ERATE, "LSD backward")
        state = torch.empty(nfloats, dtype=torch.float32, device=grad.device)
        rc = lib.fsem_lsd_grad_rate_f32(ctx.clean.data_ptr(), ctx.noisy.data_ptr(), B, L, ctx.clean.stride(0),
                                        _native.ptr(ctx.lens), ctx.sr, g[0].data_ptr(), state.data_ptr(),
                                        grad.data_ptr(), grad.stride(0), _native.stream_handle(grad.device))
        _native.check(rc, "LSD backward")
        return grad, None, None, None, None, None


class LSD(BaseMetric):
    higher_is_better = False
    EXPECTED_SAMPLING_RATE = 16000
    KEYS = ("LSD",)

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, devices=None):
        super().__init__(sample_rate, use_gpu, devices=devices)
        if use_gpu:
            _native.load_lsd()  # (a missing engine raises here, not at the first call)
        self.nfft = int(self.EXPECTED_SAMPLING_RATE * 0.032)
        self.hop = int(self.EXPECTED_SAMPLING_RATE * 0.016)
        self.p = 2
        self.eps = 1e-8

    @property
    def window(self) -> torch.Tensor:
        """[512] float32 periodic Hann window (LSD.py:16), on the metric's device."""
        return torch.hann_window(self.nfft, device=self.home_device())

    def scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, sample_rate: int | None = None,
               lengths=None) -> torch.Tensor:
        """lsd [B] float32 tensor on the metric's device, without a host sync.

        Rows at ``sample_rate``; None means rows already at 16 kHz, which requires a 16 kHz metric
        (``LSD(8000).scores`` must be told its rows' rate).  Other rates are resampled to 16 kHz
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
        """lsd [B] of rows at rate ``sr`` on their own device (one engine call)."""
        if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        if sr != self.EXPECTED_SAMPLING_RATE:
            clean_speech, denoised_speech, lengths = resample_rows(clean_speech, denoised_speech, lengths, sr,
                                                                   self.EXPECTED_SAMPLING_RATE)
        clean, noisy = pair_rows(clean_speech, denoised_speech)
        B, L = clean.shape
        if not clean.is_cuda:
            if lengths is not None:
                return _cpu.per_row(_cpu.lsd, clean, noisy, device_lengths(lengths, B, L, "cpu"))
            return _cpu.rows_parallel(_cpu.lsd, clean, noisy)
        # (the engine takes rows of at least one sample: a row of none is zero samples of length 0)
        clean, noisy, L, lens = engine_rows(clean, noisy, lengths, empty_as_zeros=True)
        return _engine_scores(clean, noisy, B, L, lens)

    # ------------------------------------------------------------------ scores to train against
    def _differentiable(self, clean_speech, denoised_speech, sample_rate, lengths) -> torch.Tensor:
        """lsd [B] with the graph to ``denoised_speech`` (include/fsem.h, "LSD with gradients"): float32
        from the engine on CUDA rows, float64 from ``_cpu.lsd64`` under torch's own autograd on host rows."""
        if self._fanout is not None:
            raise NotImplementedError("LSD: devices= is not supported with gradients (the multi-device fan-out "
                                      "returns detached scores)")
        sr = check_row_rate(self, sample_rate)
        clean, noisy = grad_operands(self, clean_speech, denoised_speech)
        if not clean.is_cuda:
            return self._differentiable_cpu(clean, noisy, sr, lengths)
        _native.load_lsd()
        if clean.shape[1] == 0:  # rows of no samples: the scores, and an empty gradient
            return self._rows_scores(clean, noisy.detach(), sr, lengths) + noisy.to(torch.float32).sum(1) * 0
        # (rows at another rate stay at that rate: the backward resamples them itself, in double)
        clean, rows, L, lens = grad_engine_rows(clean, noisy, lengths)
        return _EngineScores.apply(rows, clean, lens, L, sr, self)

    def _differentiable_cpu(self, clean, noisy, sr: int, lengths) -> torch.Tensor:
        B, L = clean.shape
        lens = device_lengths(lengths, B, L, "cpu").tolist() if lengths is not None else [L] * B
        nan = torch.full((1,), float("nan"), dtype=torch.float64)
        out = []
        for b in range(B):  # (a plain loop: each row's graph hangs on its own slice of `noisy`)
            n = int(lens[b])
            c, row = clean[b:b + 1, :n], noisy[b:b + 1, :n]
            if not bool(torch.isfinite(c).all() and torch.isfinite(row.detach()).all()):
                out.append(nan)  # a non-finite sample: NaN, no gradient (a zero row)
                continue
            out.append(_cpu.lsd64(_cpu.resample64(c, sr, self.EXPECTED_SAMPLING_RATE),
                                  _cpu.resample64(row, sr, self.EXPECTED_SAMPLING_RATE)))
        return torch.cat(out) if B else torch.zeros(0, dtype=torch.float64)

    def differentiable_scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor,
                              sample_rate: int | None = None, lengths=None) -> torch.Tensor:
        """lsd [B] as ``scores``, carrying the gradient with respect to ``denoised_speech``: float32 and
        bitwise ``scores()`` on the engine, float64 in CPU mode.  The engine's backward is
        ``fsem_lsd_grad_f32``; at other rates ``fsem_lsd_grad_rate_f32``, which resamples in double and
        differentiates at those rows.  The clean rows are constants; a row with a non-finite sample (NaN)
        gets a zero gradient; a zero estimate magnitude and a zero frame value take the subgradient 0, so a
        silent estimate has an exactly zero gradient."""
        return self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)

    def loss(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, sample_rate: int | None = None,
             lengths=None) -> torch.Tensor:
        """+mean of LSD (lower is better) over the rows with a finite score: a scalar that carries the
        gradient with respect to ``denoised_speech``.  With no such row: a zero with a zero gradient."""
        lsd = self._differentiable(clean_speech, denoised_speech, sample_rate, lengths)
        mean, _ = scored_mean(lsd, torch.isfinite(lsd.detach()), denoised_speech)
        return mean

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            lsd = self.scores(clean_speech, denoised_speech, self.EXPECTED_SAMPLING_RATE, lengths=lengths)
            return self.result_list(lsd.float().reshape(1, -1))
