"""LSD metric -- drop-in for the reference's ``fast_se_metrics.LSD`` (LSD.py:6-52), the
log-spectral distance of the URGENT challenge's evaluation.

Rows are scored at 16 kHz (other rates go through BaseMetric's resampler, as for PESQ): the
denoised row is scaled onto the clean one, both get a centred 512-point STFT (hop 256, periodic
Hann window), and the score is the mean over frames of the root mean square over the 257 bins of
``ln(S^2 / (H + 1e-8)^2 + 1e-8)`` (include/fsem_lsd.h).  ``use_gpu=True``: one engine call
(``fsem_lsd_f32``, csrc/lsd.hip, in libfsem_lsd.so); ``use_gpu=False``: the package's CPU
implementation (``_cpu.lsd``).  No warnings or exceptions for silent or empty rows: they score as
the definition says (ln 1e8 = 18.42068 for a silent clean row or a row of no samples).
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import (BaseMetric, check_row_rate, device_lengths, engine_rows, noisy_shape, pair_rows, resample_rows)


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
        lib = _native.load_lsd()
        # (the engine takes rows of at least one sample: a row of none is zero samples of length 0)
        clean, noisy, L, lens = engine_rows(clean, noisy, lengths, empty_as_zeros=True)
        out = torch.empty(B, dtype=torch.float32, device=clean.device)
        if B == 0:
            return out
        ws = _native.workspace(lib.fsem_lsd_workspace_bytes(B, L), clean.device)
        rc = lib.fsem_lsd_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0),
                              _native.ptr(lens), out.data_ptr(), ws.data_ptr(),
                              ws.numel(), _native.stream_handle(clean.device))
        _native.check(rc, "LSD")
        return out

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            lsd = self.scores(clean_speech, denoised_speech, self.EXPECTED_SAMPLING_RATE, lengths=lengths)
            return self.result_list(lsd.float().reshape(1, -1))
