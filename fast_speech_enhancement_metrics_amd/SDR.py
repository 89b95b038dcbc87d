"""SDR metric -- SI-SDR, SNR and segmental SNR of (clean, denoised) pairs, in dB.

An extension: the reference has no energy-ratio metric.  The definitions are those of
include/fsem.h ("SDR"): rows are scored at the metric's own ``sample_rate`` (no resampling);
SI-SDR after Le Roux et al. 2019 (``zero_mean=True`` removes each row's mean first), SNR =
10 log10(sum s^2 / sum (s^ - s)^2), segmental SNR with Hu & Loizou's parameters (30 ms
window, 7.5 ms hop, per-frame values clamped to [-10, 35] dB).  ``use_gpu=True``: one engine
call (``fsem_sdr_f32``, csrc/sdr.hip) that reads each input once; ``use_gpu=False``: the
package's float64 CPU implementation (``_cpu.sdr``).  No warnings or exceptions for short or
silent rows: they score NaN / +-inf as the definitions say.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import BaseMetric, device_lengths, engine_rows, noisy_shape, pair_rows


class SDR(BaseMetric):
    higher_is_better = True
    KEYS = ("SI-SDR", "SNR", "SegSNR")

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, zero_mean: bool = False, devices=None):
        # rows are scored at the rate they come in: BaseMetric's resampler is the identity
        self.EXPECTED_SAMPLING_RATE = int(sample_rate)
        self.zero_mean = bool(zero_mean)
        hop, _ = _cpu.sdr_geometry(sample_rate)
        if not 4000 <= int(sample_rate) <= 192000:
            raise NotImplementedError(f"unsupported sample rate {sample_rate}: SDR takes 4000 ... 192000 Hz "
                                      "(include/fsem.h, FSEM_ERATE)")
        super().__init__(int(sample_rate), use_gpu, devices=devices)
        self.hop_length = hop
        self.win_length = 4 * hop

    def scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, lengths=None):
        """(si_sdr [B], snr [B], seg_snr [B]) float32 tensors on the metric's device, without a host
        sync.  ``lengths`` (optional, [B] ints): row b holds lengths[b] samples and scores as the
        unpadded row alone would."""
        if self.fans_out():
            if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
                raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
            return self.fan_out(self._rows_scores, clean_speech, denoised_speech, lengths, 3, balance=lengths)
        return self._rows_scores(clean_speech, denoised_speech, lengths)

    def _rows_scores(self, clean_speech, denoised_speech, lengths):
        """The three [B] score tensors of rows on their own device (one engine call)."""
        clean, noisy = pair_rows(clean_speech, denoised_speech)
        B, L = clean.shape
        sr = self.sample_rate
        if not clean.is_cuda:
            fn = lambda c, n: _cpu.sdr(c, n, sr, self.zero_mean)  # noqa: E731
            if lengths is not None:
                out = _cpu.per_row(fn, clean, noisy, device_lengths(lengths, B, L, "cpu"))
            else:
                out = _cpu.rows_parallel(fn, clean, noisy)
            return tuple(v.to(torch.float32) for v in out)
        lib = _native.load()
        clean, noisy, L, lens = engine_rows(clean, noisy, lengths)
        out = torch.empty(3, B, dtype=torch.float32, device=clean.device)
        if L == 0:  # (no samples in any row: nothing to launch)
            return tuple(out.fill_(float("nan")))
        ws = _native.workspace(lib.fsem_sdr_workspace_bytes(B, L, sr), clean.device)
        rc = lib.fsem_sdr_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0),
                              _native.ptr(lens), sr, int(self.zero_mean),
                              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(),
                              _native.stream_handle(clean.device))
        _native.check(rc, "SDR")
        return out[0], out[1], out[2]

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            cols = self.scores(clean_speech, denoised_speech, lengths=lengths)
            return self.result_list(torch.stack([c.float() for c in cols]))
