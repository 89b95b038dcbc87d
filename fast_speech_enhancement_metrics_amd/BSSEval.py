"""BSSEval metric -- SDR, SIR and SAR of E estimates against the S sources of a mixture, the energy
ratios of ``mir_eval.separation.bss_eval_sources`` with a 512-tap distortion filter (the quantity
of ``fast_bss_eval.bss_eval_sources``).  An extension: the reference has no such metric; ``BSSSDR``
(the reference's ``SDR``) is its one-source SDR.

The definition is that of include/fsem.h ("BSS-eval").  Mixtures are
scored at 16 kHz (other rates are resampled first, each row as the row alone): every row is scaled
to unit norm, each estimate is projected on the 512 delays of each source (``coh``) and of all sources
together (``coh_all``), and ``SDR = coh / (1 - coh)``, ``SIR = coh / (coh_all - coh)``,
``SAR = coh_all / (1 - coh_all)`` in dB.  With ``permutation="SIR"`` (mir_eval's rule) or ``"SDR"`` and
as many estimates as sources, the estimates are assigned to the sources so that the mean of that
score is largest.  ``use_gpu=True``: two engine calls (``fsem_bsseval_f32``,
``fsem_bsseval_scores_f32``, csrc/bsseval.hip); ``use_gpu=False``: the package's CPU implementation
(``_cpu.bsseval``).  A mixture with a non-finite sample, a silent source, fewer than 512 S - 511 samples
or a singular system scores NaN, in that mixture only.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import BaseMetric, check_row_rate, device_lengths, resample_rows


class BSSEval(BaseMetric):
    higher_is_better = True
    EXPECTED_SAMPLING_RATE = 16000
    KEYS = ("SDR", "SIR", "SAR")
    MAX_SOURCES = _cpu.BSSEVAL_MAX_SOURCES

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, permutation="SIR", devices=None):
        if devices is not None:
            raise NotImplementedError("BSSEval: devices= is not supported (the multi-device fan-out splits 2-D "
                                      "row pairs, not mixtures)")
        if permutation not in _cpu.BSSEVAL_CRITERIA:
            raise ValueError(f"permutation must be one of {list(_cpu.BSSEVAL_CRITERIA)}, not {permutation!r}")
        super().__init__(sample_rate, use_gpu)
        self.permutation = permutation
        self.filter_length = 512

    # ------------------------------------------------------------------ inputs
    def _mixtures(self, sources, estimates):
        """(sources [B, S, L], estimates [B, E, L]) float32 on one device; 2-D inputs are S = E = 1."""
        if isinstance(sources, (list, tuple)) or isinstance(estimates, (list, tuple)):
            raise NotImplementedError("BSSEval: lists of utterances are not supported; pass padded [B, S, L] and "
                                      "[B, E, L] tensors with lengths=")
        s, h = torch.as_tensor(sources), torch.as_tensor(estimates)
        if s.dim() <= 2 and h.dim() <= 2:
            s, h = torch.atleast_2d(s)[:, None], torch.atleast_2d(h)[:, None]
        if s.dim() != 3 or h.dim() != 3 or s.shape[0] != h.shape[0] or s.shape[2] != h.shape[2]:
            raise Exception("`sources` [B, S, L] and `estimates` [B, E, L] should share the batch and the length.")
        S, E = s.shape[1], h.shape[1]
        if not (1 <= S <= self.MAX_SOURCES and 1 <= E <= S):
            raise ValueError(f"BSSEval takes 1 ... {self.MAX_SOURCES} sources and 1 ... S estimates, not S = {S}, "
                             f"E = {E}")
        dev = self.device if not s.is_cuda else s.device
        return s.to(dev, torch.float32), h.to(dev, torch.float32)

    def _at_16k(self, x, lengths, sr: int):
        """[B, R, L] rows at rate sr -> the same at 16 kHz, each row resampled as the row alone, and the
        mixtures' lengths there."""
        B, R, L = x.shape
        rows = x.reshape(B * R, L)
        lens = None
        if lengths is not None:
            lens = device_lengths(lengths, B, L, rows.device).repeat_interleave(R)
        _, rows, lens = resample_rows(None, rows, lens, sr, self.EXPECTED_SAMPLING_RATE)
        return rows.reshape(B, R, -1), (lens.reshape(B, R)[:, 0].contiguous() if lens is not None else None)

    # ------------------------------------------------------------------ scores
    def scores(self, sources, estimates, sample_rate: int | None = None, lengths=None, mixture=None,
               return_matrix: bool = False):
        """(sdr, sir, sar [B, E] float32, perm [B, E] int32) on the metric's device, without a host sync:
        estimate e against source perm[b, e].  ``return_matrix``: also the [B, S, E] SDR and SIR of every
        (source, estimate) pair.  ``mixture`` [B, L]: also SDRi [B, E] = SDR[perm[e], e] - SDR(perm[e],
        mixture), the improvement over the unprocessed mixture (last).

        Rows at ``sample_rate`` (None: rows at 16 kHz, which requires a 16 kHz metric).  ``lengths``
        (optional, [B] ints at that rate): mixture b holds lengths[b] samples and scores as the
        unpadded mixture alone would."""
        sr = check_row_rate(self, sample_rate)
        s, h = self._mixtures(sources, estimates)
        mix = None
        if mixture is not None:
            mix = torch.atleast_2d(torch.as_tensor(mixture)).to(s.device, torch.float32)[:, None]
            if mix.shape[0] != s.shape[0] or mix.shape[2] != s.shape[2]:
                raise Exception("`mixture` [B, L] should share the batch and the length of `sources`.")
        lens = lengths
        if sr != self.EXPECTED_SAMPLING_RATE:
            s, lens = self._at_16k(s, lengths, sr)
            h, _ = self._at_16k(h, lengths, sr)
            if mix is not None:
                mix, _ = self._at_16k(mix, lengths, sr)
        B, L = s.shape[0], s.shape[2]
        if lens is not None:
            lens = device_lengths(lens, B, L, s.device)
        coh, coh_all = self._energies(s, h, lens)
        out = self._from_energies(coh, coh_all, self.permutation, True)
        res = out[:6] if return_matrix else out[:4]
        if mix is not None:
            base = self._from_energies(*self._energies(s, mix, lens), None, True)[4]  # [B, S, 1]
            res = res + (out[0] - base[:, :, 0].gather(1, out[3].long()),)
        return res

    def _energies(self, s: torch.Tensor, h: torch.Tensor, lens):
        """(coh [B, S, E], coh_all [B, E]) float64 of float32 mixtures at 16 kHz on their device."""
        B, S, L = s.shape
        E = h.shape[1]
        if not s.is_cuda:
            return _cpu.bsseval(s, h, lens)
        if L == 0:  # (the engine takes rows of at least one sample: one zero sample, of length 0)
            s, h, L = s.new_zeros(B, S, 1), h.new_zeros(B, E, 1), 1
            lens = torch.zeros(B, dtype=torch.int32, device=s.device)
        s, h = s.contiguous(), h.contiguous()
        return self.engine_energies(s, h, B, S, E, L, L, lens)[:2]

    @staticmethod
    def engine_energies(src: torch.Tensor, est: torch.Tensor, B: int, S: int, E: int, L: int, ld: int, lens):
        """One fsem_bsseval_f32 call on device rows (row (b, i) at (b S + i) ld): (coh, coh_all, norms
        [B, S + E] float32, corr [B, corr_doubles] float64)."""
        lib = _native.load()
        dev = src.device
        coh = torch.empty(B, S, E, dtype=torch.float64, device=dev)
        coh_all = torch.empty(B, E, dtype=torch.float64, device=dev)
        norms = torch.empty(B, S + E, dtype=torch.float32, device=dev)
        corr = torch.empty(B, lib.fsem_bsseval_corr_doubles(S, E, L), dtype=torch.float64, device=dev)
        rc = lib.fsem_bsseval_f32(src.data_ptr(), est.data_ptr(), B, S, E, L, ld,
                                  _native.ptr(lens), norms.data_ptr(), corr.data_ptr(),
                                  coh.data_ptr(), coh_all.data_ptr(), _native.stream_handle(dev))
        _native.check(rc, "BSSEval")
        return coh, coh_all, norms, corr

    @staticmethod
    def _from_energies(coh: torch.Tensor, coh_all: torch.Tensor, criterion, matrices: bool):
        """(sdr, sir, sar, perm, sdr_mat, sir_mat) of the energies, on their device."""
        if not coh.is_cuda:
            return _cpu.bsseval_scores(coh, coh_all, criterion)
        B, S, E = coh.shape
        dev = coh.device
        sdr, sir, sar = (torch.empty(B, E, dtype=torch.float32, device=dev) for _ in range(3))
        perm = torch.empty(B, E, dtype=torch.int32, device=dev)
        sdm, sim = (torch.empty(B, S, E, dtype=torch.float32, device=dev) if matrices else None for _ in range(2))
        rc = _native.load().fsem_bsseval_scores_f32(
            coh.data_ptr(), coh_all.data_ptr(), B, S, E, _cpu.BSSEVAL_CRITERIA[criterion], sdr.data_ptr(),
            sir.data_ptr(), sar.data_ptr(), perm.data_ptr(), _native.ptr(sdm), _native.ptr(sim),
            _native.stream_handle(dev))
        _native.check(rc, "BSSEval scores")
        return sdr, sir, sar, perm, sdm, sim

    # ------------------------------------------------------------------ the drop-in call
    def compute_metric(self, clean_speech, denoised_speech, lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            sdr, sir, sar, _ = self.scores(clean_speech, denoised_speech, self.sample_rate, lengths=lengths)
            return self.result_list(torch.stack([sdr.mean(1), sir.mean(1), sar.mean(1)]).float().contiguous())

    def __call__(self, sources, estimates, lengths=None) -> list[dict[str, float]]:
        """One dict per mixture, {"SDR", "SIR", "SAR"}: the means over the mixture's estimates.  Rows at the
        metric's ``sample_rate``; ``lengths``: [B] ints, one per mixture."""
        return self.compute_metric(sources, estimates, lengths)
