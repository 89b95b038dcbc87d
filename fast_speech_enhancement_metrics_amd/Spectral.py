"""SpectralMeasures -- the frequency-weighted segmental SNR (fwSegSNR), the LPC cepstral distance
(CD) and the Itakura-Saito distance (IS) of (clean, denoised) pairs, from Hu & Loizou's evaluation set.

An extension: the reference has no such measure.  The definitions are those of include/fsem.h
("Spectral"), on Composite's frames (30 ms window, 7.5 ms hop), LPC
orders and band filters, at the metric's own ``sample_rate`` (8000 or 16000 Hz).  CD and IS are
the mean of the lowest 95 % of the frame values, fwSegSNR the mean of all frames (NaN when a clean
frame is digitally silent: take your own mean of the frame values then).  ``use_gpu=True``: one
engine call (``fsem_spectral_f32``, csrc/spectral.hip); ``use_gpu=False``: the package's float64
CPU implementation (``_cpu.spectral``).  No implementation of Loizou's ``comp_fwseg.m``,
``comp_cep.m`` and ``comp_is.m`` was available to compare with: agreement with them is by
definition only.

``higher_is_better`` is per key: True for fwSegSNR, False for CD and IS.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import BaseMetric, device_lengths, noisy_shape, pair_rows


class SpectralMeasures(BaseMetric):
    higher_is_better = {"fwSegSNR": True, "CD": False, "IS": False}
    KEYS = ("fwSegSNR", "CD", "IS")

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, devices=None):
        if int(sample_rate) not in (8000, 16000):
            raise NotImplementedError(f"unsupported sample rate {sample_rate}: SpectralMeasures takes 8000 or 16000 Hz "
                                      "(include/fsem.h, FSEM_ERATE)")
        # rows are scored at the rate they come in: BaseMetric's resampler is the identity
        self.EXPECTED_SAMPLING_RATE = int(sample_rate)
        super().__init__(int(sample_rate), use_gpu, devices=devices)
        self.hop_length, self.win_length = _cpu.sdr_geometry(sample_rate)
        self.lpc_order = _cpu.composite_order(sample_rate)

    def frames_of(self, n: int) -> int:
        """Complete frames of a row of n samples."""
        return (int(n) - self.win_length) // self.hop_length + 1 if n >= self.win_length else 0

    def scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, lengths=None,
               return_frames: bool = False):
        """(fwsegsnr, cd, is): three [B] float32 tensors on the metric's device, without a host
        sync.  ``lengths`` (optional, [B] ints): row b holds lengths[b] samples and scores as the
        unpadded row alone would.  ``return_frames``: also the [3, B, F] float32 frame values
        (fwSegSNR_f, CD_f, IS_f; F of the row capacity, NaN past a shorter row's own frames); a
        multi-device metric then scores the call on its first device alone."""
        if self.fans_out() and not return_frames:
            if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
                raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
            return self.fan_out(self._rows_scores, clean_speech, denoised_speech, lengths, 3, balance=lengths)
        if self.devices is not None:
            home = self.home_device()
            with torch.cuda.device(home):
                return self._rows_scores(torch.atleast_2d(clean_speech).to(home), torch.atleast_2d(denoised_speech).to(home),
                                         lengths, return_frames)
        return self._rows_scores(clean_speech, denoised_speech, lengths, return_frames)

    def _rows_scores(self, clean_speech, denoised_speech, lengths, return_frames: bool = False):
        """The three [B] score tensors of rows on their own device (one engine call)."""
        clean, noisy = pair_rows(clean_speech, denoised_speech)
        B, L = clean.shape
        sr = self.sample_rate
        F = self.frames_of(L)
        if not clean.is_cuda:
            return self._cpu_scores(clean, noisy, lengths, F, return_frames)
        lib = _native.load()
        # (the entry reads 4 bytes at a time at any alignment: no padding; one row stride for both)
        lens = device_lengths(lengths, B, L, clean.device) if lengths is not None else None
        if clean.stride(0) != noisy.stride(0):
            clean, noisy = clean.contiguous(), noisy.contiguous()
        out = torch.empty(3, B, dtype=torch.float32, device=clean.device)
        ldf = max(F, 1)
        if return_frames and lens is not None:  # (entries past a row's own frames stay NaN)
            frames = torch.full((3, B, ldf), float("nan"), dtype=torch.float32, device=clean.device)
        else:
            frames = torch.empty(3, B, ldf, dtype=torch.float32, device=clean.device)
        if L == 0 or B == 0:  # (no samples in any row: nothing to launch)
            out.fill_(float("nan"))
        else:
            rc = lib.fsem_spectral_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0),
                                       _native.ptr(lens), sr, frames.data_ptr(), ldf,
                                       *(out[k].data_ptr() for k in range(3)), _native.stream_handle(clean.device))
            _native.check(rc, "SpectralMeasures")
        cols = tuple(out[k] for k in range(3))
        return cols + (frames[:, :, :F],) if return_frames else cols

    def _cpu_scores(self, clean, noisy, lengths, F: int, return_frames: bool):
        sr = self.sample_rate
        B, L = clean.shape
        if lengths is None:
            if return_frames:
                out = _cpu.spectral(clean, noisy, sr, return_frames=True)
            else:
                out = _cpu.rows_parallel(lambda c, n: _cpu.spectral(c, n, sr), clean, noisy) if B else \
                    _cpu.spectral(clean, noisy, sr)
            return tuple(v.to(torch.float32) for v in out)
        lens = device_lengths(lengths, B, L, "cpu")
        cols = torch.full((3, B), float("nan"), dtype=torch.float64)
        frames = torch.full((3, B, F), float("nan"), dtype=torch.float64)
        for b in range(B):
            n = int(lens[b])
            got = _cpu.spectral(clean[b:b + 1, :n], noisy[b:b + 1, :n], sr, return_frames=True)
            cols[:, b] = torch.stack([g[0] for g in got[:3]])
            frames[:, b, :got[3].shape[2]] = got[3][:, 0]
        out = tuple(cols[k].to(torch.float32) for k in range(3))
        return out + (frames.to(torch.float32),) if return_frames else out

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            cols = self.scores(clean_speech, denoised_speech, lengths=lengths)
            return self.result_list(torch.stack([c.float() for c in cols]))
