"""SRMR -- the speech-to-reverberation modulation energy ratio (Falk, Zheng & Chan 2010), a
no-reference measure of reverberation and noise in a denoised row.

An extension: the reference has no such measure.  The definition is that of include/fsem.h ("SRMR";
INTEGRATION.md section 13): SRMRpy's full path (23 gammatone channels from 125 Hz, 8 modulation
filters from 4 to 128 Hz, 256 ms Hamming frames every 64 ms, the 90 % bandwidth rule, no
normalisation) at the metric's own ``sample_rate`` (8000 or 16000 Hz), with the temporal envelope
taken as the magnitude of an analytic (complex) gammatone instead of a whole-row Hilbert transform.
``use_gpu=True``: one engine call (``fsem_srmr_f32``, csrc/srmr.hip); ``use_gpu=False``: the
package's float64 CPU implementation (``_cpu.srmr``).

``differentiable_scores`` and ``loss`` are the same scores with the gradient with respect to the rows
(include/fsem.h, "SRMR with gradients"; K* is taken as a constant): on the
engine ``fsem_srmr_f32`` forward and ``fsem_srmrgrad_f32`` backward (csrc/srmr_grad.hip), which keeps
the energies and nothing else of the forward; in CPU mode ``_cpu.srmr64`` in float64.

``clean`` is not used: ``metric(None, denoised)`` and ``metric(clean, denoised)`` give the same scores;
a ``clean`` of another shape raises the reference's exception.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import BaseMetric, as_rows, device_lengths, grad_operands, noisy_shape, scored_mean


class _EngineScores(torch.autograd.Function):
    """SRMR [B] float32 of CUDA float32 rows (unit stride along time) by the engine, bitwise ``scores``
    (fsem_srmr_f32).  It keeps the rows, the lengths and the energies; the backward is one
    fsem_srmrgrad_f32 call on them and a scratch of its own."""

    @staticmethod
    def forward(ctx, rows, lens, sr):
        B, L = rows.shape
        lib = _native.load()
        out = torch.empty(B, dtype=torch.float32, device=rows.device)
        energies = torch.empty(B, SRMR.CHANNELS, SRMR.MODS, dtype=torch.float64, device=rows.device)
        rc = lib.fsem_srmr_f32(rows.data_ptr(), B, L, rows.stride(0), _native.ptr(lens), sr, energies.data_ptr(),
                               out.data_ptr(), _native.stream_handle(rows.device))
        _native.check(rc, "SRMR")
        ctx.rows, ctx.lens, ctx.energies, ctx.sr = rows.detach(), lens, energies, sr
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_srmr):
        rows = ctx.rows
        B, L = rows.shape
        ld = rows.stride(0)
        lib = _native.load()
        g = g_srmr.to(torch.float32).contiguous()
        # (the entry writes the gradient with the rows' own stride)
        grad = torch.empty(B, ld, dtype=torch.float32, device=rows.device)[:, :L]
        scratch = _native.workspace(lib.fsem_srmrgrad_scratch_bytes(B, L), rows.device)
        rc = lib.fsem_srmrgrad_f32(rows.data_ptr(), B, L, ld, _native.ptr(ctx.lens), ctx.sr,
                                   ctx.energies.data_ptr(), g.data_ptr(), scratch.data_ptr(), grad.data_ptr(),
                                   _native.stream_handle(rows.device))
        _native.check(rc, "SRMR backward")
        return grad, None, None


class SRMR(BaseMetric):
    higher_is_better = True
    KEYS = ("SRMR",)
    CHANNELS, MODS = _cpu.SRMR_CHANNELS, _cpu.SRMR_MODS
    TILE = 4096  # samples the engine stages at a time (csrc/srmr.hip)

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, devices=None):
        if int(sample_rate) not in (8000, 16000):
            raise NotImplementedError(f"unsupported sample rate {sample_rate}: SRMR takes 8000 or 16000 Hz "
                                      "(include/fsem.h, FSEM_ERATE)")
        # rows are scored at the rate they come in: BaseMetric's resampler is the identity
        self.EXPECTED_SAMPLING_RATE = int(sample_rate)
        super().__init__(int(sample_rate), use_gpu, devices=devices)
        self.hop_length, self.win_length = _cpu.srmr_geometry(sample_rate)

    def frames_of(self, n: int) -> int:
        """Complete frames of a row of n samples."""
        return (int(n) - self.win_length) // self.hop_length + 1 if n >= self.win_length else 0

    def scores(self, denoised_speech: torch.Tensor, lengths=None, return_energies: bool = False):
        """SRMR: a [B] float32 tensor on the metric's device, without a host sync.  ``lengths``
        (optional, [B] ints): row b holds lengths[b] samples and scores as the unpadded row alone
        would.  ``return_energies``: also the [B, 23, 8] float64 modulation energies A[i, k] (NaN for
        a row without a frame); a multi-device metric then scores the call on its first device alone."""
        if self.fans_out() and not return_energies:
            return self.fan_out(lambda c, n, lk: (self._rows_scores(n, lk),), denoised_speech, denoised_speech,
                                lengths, 1, balance=lengths)[0]
        if self.devices is not None:
            home = self.home_device()
            with torch.cuda.device(home):
                return self._rows_scores(torch.atleast_2d(denoised_speech).to(home), lengths, return_energies)
        return self._rows_scores(denoised_speech, lengths, return_energies)

    def _rows_scores(self, denoised_speech, lengths, return_energies: bool = False):
        """The [B] scores of rows on their own device (one engine call)."""
        rows = as_rows(denoised_speech)
        B, L = rows.shape
        if not rows.is_cuda:
            return self._cpu_scores(rows, lengths, return_energies)
        lib = _native.load()
        # (the entry reads 4 bytes at a time at any alignment: no padding, no copy of a strided view)
        lens = device_lengths(lengths, B, L, rows.device) if lengths is not None else None
        out = torch.empty(B, dtype=torch.float32, device=rows.device)
        energies = torch.empty(B, self.CHANNELS, self.MODS, dtype=torch.float64, device=rows.device)
        if B:
            rc = lib.fsem_srmr_f32(rows.data_ptr(), B, L, rows.stride(0), _native.ptr(lens),
                                   self.sample_rate, energies.data_ptr(), out.data_ptr(),
                                   _native.stream_handle(rows.device))
            _native.check(rc, "SRMR")
        return (out, energies) if return_energies else out

    def _cpu_scores(self, rows, lengths, return_energies: bool):
        sr = self.sample_rate
        B, L = rows.shape
        if lengths is None:
            if return_energies or not B:
                score, A = _cpu.srmr(rows, sr, return_energies=True)
            else:
                score, A = _cpu.rows_parallel(lambda r, _: _cpu.srmr(r, sr), rows, rows), None
        else:
            lens = device_lengths(lengths, B, L, "cpu")
            got = [_cpu.srmr(rows[b:b + 1, :int(lens[b])], sr, return_energies=True) for b in range(B)]
            score = torch.cat([g[0] for g in got]) if B else torch.zeros(0, dtype=torch.float64)
            A = torch.cat([g[1] for g in got]) if B else torch.zeros(0, self.CHANNELS, self.MODS, dtype=torch.float64)
        score = score.to(torch.float32)
        return (score, A) if return_energies else score

    # ------------------------------------------------------------------ scores to train against
    def _differentiable(self, denoised_speech, lengths) -> torch.Tensor:
        """SRMR [B] with the graph to ``denoised_speech``: float32 from the engine on CUDA rows, float64 from
        ``_cpu.srmr64`` on host rows."""
        if self._fanout is not None:
            raise NotImplementedError("SRMR: devices= is not supported with gradients (the multi-device fan-out "
                                      "returns detached scores)")
        _, noisy = grad_operands(self, torch.as_tensor(denoised_speech).detach(), denoised_speech)
        B, L = noisy.shape
        if not noisy.is_cuda:
            lens = device_lengths(lengths, B, L, "cpu").tolist() if lengths is not None else [L] * B
            # (a plain loop: each row's graph hangs on its own slice of `noisy`)
            out = [_cpu.srmr64(noisy[b:b + 1, :int(lens[b])], self.sample_rate) for b in range(B)]
            return torch.cat(out) if B else torch.zeros(0, dtype=torch.float64)
        _native.load()
        if B == 0 or L == 0:  # nothing to launch: the scores (NaN: no row has a frame), and an empty gradient
            nan = torch.full((B,), float("nan"), dtype=torch.float32, device=noisy.device)
            return nan + noisy.to(torch.float32).sum(1) * 0
        rows = noisy.to(torch.float32)
        if rows.stride(-1) != 1 or rows.stride(0) < L:
            rows = rows.contiguous()
        lens = device_lengths(lengths, B, L, rows.device) if lengths is not None else None
        return _EngineScores.apply(rows, lens, self.sample_rate)

    def differentiable_scores(self, denoised_speech: torch.Tensor, lengths=None) -> torch.Tensor:
        """SRMR [B] as ``scores``, carrying the gradient with respect to ``denoised_speech``: float32 and
        bitwise ``scores()`` on the engine (backward: ``fsem_srmrgrad_f32``), float64 in CPU mode.  K* is
        taken as a constant.  A row without a frame, with a non-finite sample or with a non-finite score (a
        digitally silent row) gets a zero gradient; the gradient is zero from the last frame's end - 1 on and
        past ``lengths``; |y| = 0 takes the subgradient 0."""
        return self._differentiable(denoised_speech, lengths)

    def loss(self, denoised_speech: torch.Tensor, lengths=None) -> torch.Tensor:
        """-mean of SRMR (higher is better) over the rows with a finite score: a scalar that carries the
        gradient with respect to ``denoised_speech``.  With no such row: a zero with a zero gradient."""
        score = self._differentiable(denoised_speech, lengths)
        mean, _ = scored_mean(score, torch.isfinite(score.detach()), denoised_speech)
        return -mean

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        if clean_speech is not None and noisy_shape(clean_speech) != noisy_shape(denoised_speech):
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        with torch.no_grad():
            s = self.scores(denoised_speech, lengths=lengths)
            return self.result_list(s.float()[None, :].contiguous())  # [1, B]
