"""Composite metric -- CSIG, CBAK, COVL of (clean, denoised) pairs with their ingredients PESQ, LLR,
WSS and SegSNR (Hu & Loizou 2008).

An extension: the reference has no composite measure.  The definitions are those of
include/fsem_composite.h: LLR, WSS and the segmental SNR on the
rows at the metric's own ``sample_rate`` (8000 or 16000 Hz; 30 ms window, 7.5 ms hop), LLR and WSS
as the mean of the lowest 95 % of the frame values; PESQ is this package's wideband MOS-LQO
(8 kHz rows resampled to 16 kHz, as ``PESQ`` does).  ``use_gpu=True``: one engine call
(``fsem_composite_f32``, csrc/composite.hip); ``use_gpu=False``: the package's float64 CPU
implementation (``_cpu.composite``).  Rows too short for PESQ behave as in ``PESQ``: NaN in that
row with ``lengths=`` or lists, the class's exception in the whole-batch form.  No implementation
of Loizou's ``composite.m`` was available to compare with: agreement with it is by definition only.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import BaseMetric, device_lengths, engine_rows, noisy_shape, pair_rows


class Composite(BaseMetric):
    higher_is_better = True
    KEYS = ("CSIG", "CBAK", "COVL", "PESQ", "LLR", "WSS", "SegSNR")

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, devices=None):
        if int(sample_rate) not in (8000, 16000):
            raise NotImplementedError(f"unsupported sample rate {sample_rate}: Composite takes 8000 or 16000 Hz "
                                      "(include/fsem_composite.h, FSEM_ERATE)")
        # rows are scored at the rate they come in (the engine resamples 8 kHz rows for PESQ itself):
        # BaseMetric's resampler is the identity
        self.EXPECTED_SAMPLING_RATE = int(sample_rate)
        super().__init__(int(sample_rate), use_gpu, devices=devices)
        if use_gpu:
            _native.load_composite()  # (a missing engine is an error at construction, as BaseMetric's)
        self.hop_length, self.win_length = _cpu.sdr_geometry(sample_rate)
        self.lpc_order = _cpu.composite_order(sample_rate)

    def scores(self, clean_speech: torch.Tensor, denoised_speech: torch.Tensor, lengths=None):
        """(csig, cbak, covl, pesq, llr, wss, seg_snr): seven [B] float32 tensors on the metric's
        device, without a host sync.  ``lengths`` (optional, [B] ints): row b holds lengths[b]
        samples and scores as the unpadded row alone would."""
        if self.fans_out():
            if noisy_shape(clean_speech) != noisy_shape(denoised_speech):
                raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
            return self.fan_out(self._rows_scores, clean_speech, denoised_speech, lengths, 7, balance=lengths)
        return self._rows_scores(clean_speech, denoised_speech, lengths)

    def _rows_scores(self, clean_speech, denoised_speech, lengths):
        """The seven [B] score tensors of rows on their own device (one engine call)."""
        clean, noisy = pair_rows(clean_speech, denoised_speech)
        B, L = clean.shape
        sr = self.sample_rate
        if lengths is None and _cpu.pesq_frames(L * (16000 // sr)) < 20:
            # PESQ's whole-batch form fails here (the reference's unfold(1, size=20, step=10), PESQ.py:169)
            raise RuntimeError(f"maximum size for tensor at dimension 1 is {max(_cpu.pesq_frames(L * (16000 // sr)), 0)} "
                               "but size is 20")
        if not clean.is_cuda:
            if lengths is not None:
                fn = lambda c, n: _cpu.composite(c, n, sr, short_ok=True)  # noqa: E731
                out = _cpu.per_row(fn, clean, noisy, device_lengths(lengths, B, L, "cpu"))
            else:
                out = _cpu.rows_parallel(lambda c, n: _cpu.composite(c, n, sr), clean, noisy)
            return tuple(v.to(torch.float32) for v in out)
        lib = _native.load_composite()
        # (the PESQ stage reads rows in 16-byte pieces)
        clean, noisy, L, lens = engine_rows(clean, noisy, lengths, aligned16=True)
        out = torch.empty(7, B, dtype=torch.float32, device=clean.device)
        if L == 0:  # (no samples in any row: nothing to launch)
            return tuple(out.fill_(float("nan")))
        ws = _native.workspace(lib.fsem_composite_workspace_bytes(B, L, sr), clean.device)
        rc = lib.fsem_composite_f32(clean.data_ptr(), noisy.data_ptr(), B, L, clean.stride(0),
                                    _native.ptr(lens), sr,
                                    *(out[k].data_ptr() for k in range(7)), ws.data_ptr(), ws.numel(),
                                    _native.stream_handle(clean.device))
        _native.check(rc, "Composite")
        return tuple(out[k] for k in range(7))

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            cols = self.scores(clean_speech, denoised_speech, lengths=lengths)
            return self.result_list(torch.stack([c.float() for c in cols]))
