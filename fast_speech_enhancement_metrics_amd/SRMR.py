"""SRMR -- the speech-to-reverberation modulation energy ratio (Falk, Zheng & Chan 2010), a
no-reference measure of reverberation and noise in a denoised row.

An extension: the reference has no such measure.  The definition is that of include/fsem.h ("SRMR";
INTEGRATION.md section 13): SRMRpy's full path (23 gammatone channels from 125 Hz, 8 modulation
filters from 4 to 128 Hz, 256 ms Hamming frames every 64 ms, the 90 % bandwidth rule, no
normalisation) at the metric's own ``sample_rate`` (8000 or 16000 Hz), with the temporal envelope
taken as the magnitude of an analytic (complex) gammatone instead of a whole-row Hilbert transform.
``use_gpu=True``: one engine call (``fsem_srmr_f32``, csrc/srmr.hip); ``use_gpu=False``: the
package's float64 CPU implementation (``_cpu.srmr``).

``clean`` is not used: ``metric(None, denoised)`` and ``metric(clean, denoised)`` give the same scores;
a ``clean`` of another shape raises the reference's exception.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import BaseMetric, as_rows, device_lengths, noisy_shape


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

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        if clean_speech is not None and noisy_shape(clean_speech) != noisy_shape(denoised_speech):
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        with torch.no_grad():
            s = self.scores(denoised_speech, lengths=lengths)
            return self.result_list(s.float()[None, :].contiguous())  # [1, B]
