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
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import (BaseMetric, check_row_rate, device_lengths, engine_rows, noisy_shape, pair_rows, resample_rows)


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

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            sdr = self.scores(clean_speech, denoised_speech, self.EXPECTED_SAMPLING_RATE, lengths=lengths)
            return self.result_list(sdr.float().reshape(1, -1))
