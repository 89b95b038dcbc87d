"""PITSDR metric -- the scale-invariant SDR and the SNR of E estimates against the S sources of a mixture
under the best assignment, its improvement over the unprocessed mixture (SI-SDRi), and the same
quantity as a training loss: both score matrices are differentiable with respect to the estimates.
An extension: the reference has no such metric.

The definition is that of include/fsem.h ("PITSDR").  Rows are scored at
the metric's own ``sample_rate`` (no resampling).  Per pair, SNR = 10 log10(sum s^2 / sum (s^ - s)^2) and
SI-SDR as ``SDR`` defines it (``zero_mean=True`` removes each row's mean first).  With
``permutation="SI-SDR"`` or ``"SNR"`` and as many estimates as sources, the estimates are assigned to the
sources so that the mean of that score is largest.  ``use_gpu=True``: the HIP engine (``fsem_pitsdr_f32``
forward, ``fsem_pitsdr_grad_f32`` backward, csrc/pitsdr.hip), float32 scores from sums in double;
``use_gpu=False``: float64 torch ops (``_cpu.pitsdr``) under torch's own autograd.  A mixture with a
non-finite sample or without samples scores NaN, in that mixture only; on the engine its gradient is
zero, and a pair whose score is not finite adds nothing to the gradient.
"""
from __future__ import annotations

import torch

from . import _cpu, _native
from .base import BaseMetric, device_lengths


class _EngineMatrices(torch.autograd.Function):
    """(si_mat, snr_mat [B, S, E] float32, perm [B, E] int32) of CUDA mixtures by the engine; the backward
    is fsem_pitsdr_grad_f32 on the totals the forward left in ``sums``."""

    @staticmethod
    def forward(ctx, est, src, lens, sample_rate, zero_mean, criterion):
        lib = _native.load()
        B, S, L = src.shape
        E = est.shape[1]
        dev = src.device
        si = torch.empty(B, S, E, dtype=torch.float32, device=dev)
        snr = torch.empty(B, S, E, dtype=torch.float32, device=dev)
        perm = torch.empty(B, E, dtype=torch.int32, device=dev)
        ctx.mark_non_differentiable(perm)
        ctx.shape = (B, S, E, L)
        if L == 0 or B == 0:  # (no samples in any mixture: nothing to launch)
            ctx.sums = None
            perm.copy_(torch.arange(E, dtype=torch.int32, device=dev).repeat(B, 1))
            return si.fill_(float("nan")), snr.fill_(float("nan")), perm
        (src, ld), (est, ld_est) = PITSDR.engine_rows(src), PITSDR.engine_rows(est)
        if ld != ld_est:  # (the entry takes one row stride)
            src, est, ld = src.contiguous(), est.contiguous(), L
        sums = torch.empty(B, lib.fsem_pitsdr_sums_doubles(S, E, L, sample_rate), dtype=torch.float64, device=dev)
        rc = lib.fsem_pitsdr_f32(src.data_ptr(), est.data_ptr(), B, S, E, L, ld,
                                 _native.ptr(lens), sample_rate, int(zero_mean), criterion,
                                 sums.data_ptr(), si.data_ptr(), snr.data_ptr(), perm.data_ptr(),
                                 _native.stream_handle(dev))
        _native.check(rc, "PITSDR")
        ctx.sums, ctx.src, ctx.est, ctx.lens, ctx.ld, ctx.zero_mean = sums, src, est, lens, ld, int(zero_mean)
        return si, snr, perm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_si, g_snr, _g_perm):
        B, S, E, L = ctx.shape
        dev = g_si.device
        grad = torch.empty(B, E, L, dtype=torch.float32, device=dev)
        if ctx.sums is None:
            return grad.zero_(), None, None, None, None, None
        g_si = g_si.to(torch.float32).contiguous()
        g_snr = g_snr.to(torch.float32).contiguous()
        lens = ctx.lens
        rc = _native.load().fsem_pitsdr_grad_f32(
            ctx.src.data_ptr(), ctx.est.data_ptr(), B, S, E, L, ctx.ld, _native.ptr(lens),
            ctx.zero_mean, ctx.sums.data_ptr(), g_si.data_ptr(), g_snr.data_ptr(), grad.data_ptr(), L,
            _native.stream_handle(dev))
        _native.check(rc, "PITSDR backward")
        return grad, None, None, None, None, None


class PITSDR(BaseMetric):
    higher_is_better = True
    KEYS = ("SI-SDR", "SNR")
    MAX_SOURCES = _cpu.PITSDR_MAX_SOURCES

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, zero_mean: bool = False,
                 permutation="SI-SDR", devices=None):
        if devices is not None:
            raise NotImplementedError("PITSDR: devices= is not supported (the multi-device fan-out splits 2-D "
                                      "row pairs, not mixtures)")
        if permutation not in _cpu.PITSDR_CRITERIA:
            raise ValueError(f"permutation must be one of {list(_cpu.PITSDR_CRITERIA)}, not {permutation!r}")
        if not 4000 <= int(sample_rate) <= 192000:
            raise NotImplementedError(f"unsupported sample rate {sample_rate}: PITSDR takes 4000 ... 192000 Hz "
                                      "(include/fsem.h, FSEM_ERATE)")
        # rows are scored at the rate they come in: BaseMetric's resampler is the identity
        self.EXPECTED_SAMPLING_RATE = int(sample_rate)
        super().__init__(int(sample_rate), use_gpu)
        self.zero_mean = bool(zero_mean)
        self.permutation = permutation

    # ------------------------------------------------------------------ inputs
    def _mixtures(self, sources, estimates):
        """(sources [B, S, L], estimates [B, E, L]) on one device, float32 (CPU mode keeps float64 rows as
        they are: it computes in float64); 2-D inputs are S = E = 1."""
        if isinstance(sources, (list, tuple)) or isinstance(estimates, (list, tuple)):
            raise NotImplementedError("PITSDR: lists of utterances are not supported; pass padded [B, S, L] and "
                                      "[B, E, L] tensors with lengths=")
        s, h = torch.as_tensor(sources), torch.as_tensor(estimates)
        if s.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("PITSDR: the sources are constants; gradients with respect to `sources` are "
                                      "not supported (detach them)")
        if s.dim() <= 2 and h.dim() <= 2:
            s, h = torch.atleast_2d(s)[:, None], torch.atleast_2d(h)[:, None]
        if s.dim() != 3 or h.dim() != 3 or s.shape[0] != h.shape[0] or s.shape[2] != h.shape[2]:
            raise Exception("`sources` [B, S, L] and `estimates` [B, E, L] should share the batch and the length.")
        S, E = s.shape[1], h.shape[1]
        if not (1 <= S <= self.MAX_SOURCES and 1 <= E <= S):
            raise ValueError(f"PITSDR takes 1 ... {self.MAX_SOURCES} sources and 1 ... S estimates, not S = {S}, "
                             f"E = {E}")
        dev = self.device if not s.is_cuda else s.device

        def rows(x):
            keep64 = torch.device(dev).type == "cpu" and x.dtype == torch.float64
            return x.to(dev, torch.float64 if keep64 else torch.float32)

        return rows(s.detach()), rows(h)

    @staticmethod
    def engine_rows(x: torch.Tensor):
        """([B, R, L] CUDA rows as the engine addresses them, ld): row (b, r) at (b R + r) ld.  A view that
        already is such rows (a longer capacity, one row of each mixture of a wider tensor) is not copied."""
        B, R, L = x.shape
        ld = x.stride(0) if R == 1 else x.stride(1)
        if x.stride(2) != 1 or ld < L or (R > 1 and x.stride(0) != R * ld):
            x, ld = x.contiguous(), L
        return x, ld

    # ------------------------------------------------------------------ scores
    def _matrices(self, s: torch.Tensor, h: torch.Tensor, lengths, criterion):
        """(si_mat, snr_mat [B, S, E], perm [B, E] int32): float64 in CPU mode, float32 on the engine; both
        matrices carry the gradient with respect to ``h``."""
        B, L = s.shape[0], s.shape[2]
        lens = device_lengths(lengths, B, L, s.device) if lengths is not None else None
        if not s.is_cuda:
            return _cpu.pitsdr(s, h, lens, self.zero_mean, criterion)
        return _EngineMatrices.apply(h, s, lens, self.sample_rate, self.zero_mean, _cpu.PITSDR_CRITERIA[criterion])

    @staticmethod
    def _assigned(mat: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
        """[B, E]: entry [perm[b, e], e] of a [B, S, E] matrix (a gather: autograd scatters back)."""
        return mat.gather(1, perm.long()[:, None, :])[:, 0]

    def scores(self, sources, estimates, lengths=None, mixture=None, return_matrix: bool = False):
        """(si_sdr, snr [B, E] float32, perm [B, E] int32) on the metric's device, without a host sync:
        estimate e against source perm[b, e].  ``return_matrix``: also the [B, S, E] SI-SDR and SNR of every
        (source, estimate) pair.  ``mixture`` [B, L]: also SI-SDRi [B, E] = SI-SDR[perm[e], e] -
        SI-SDR(perm[e], mixture), the improvement over the unprocessed mixture (last).

        ``lengths`` (optional, [B] ints): mixture b holds lengths[b] samples and scores as the unpadded
        mixture alone would.  Under grad mode the scores carry the gradient with respect to
        ``estimates``; ``perm`` does not."""
        s, h = self._mixtures(sources, estimates)
        si_mat, snr_mat, perm = self._matrices(s, h, lengths, self.permutation)
        si, snr = self._assigned(si_mat, perm).float(), self._assigned(snr_mat, perm).float()
        res = (si, snr, perm)
        if return_matrix:
            res = res + (si_mat.float(), snr_mat.float())
        if mixture is not None:
            mix = torch.atleast_2d(torch.as_tensor(mixture)).detach().to(s.device, s.dtype)[:, None]
            if mix.shape[0] != s.shape[0] or mix.shape[2] != s.shape[2]:
                raise Exception("`mixture` [B, L] should share the batch and the length of `sources`.")
            with torch.no_grad():
                base = self._matrices(s, mix, lengths, None)[0][:, :, 0]  # [B, S]
            res = res + ((self._assigned(si_mat, perm) - base.gather(1, perm.long())).float(),)
        return res

    def loss(self, sources, estimates, lengths=None, key: str = "SI-SDR") -> torch.Tensor:
        """-mean over (b, e) of the assigned ``key`` scores: a scalar that carries the gradient with respect
        to ``estimates`` (float32 on the engine, float64 in CPU mode)."""
        if key not in self.KEYS:
            raise ValueError(f"key must be one of {list(self.KEYS)}, not {key!r}")
        s, h = self._mixtures(sources, estimates)
        si_mat, snr_mat, perm = self._matrices(s, h, lengths, self.permutation)
        return -self._assigned(si_mat if key == "SI-SDR" else snr_mat, perm).mean()

    # ------------------------------------------------------------------ the drop-in call
    def compute_metric(self, clean_speech, denoised_speech, lengths=None) -> list[dict[str, float]]:
        assert clean_speech is not None
        with torch.no_grad():
            si, snr, _ = self.scores(clean_speech, denoised_speech, lengths=lengths)
            return self.result_list(torch.stack([si.mean(1), snr.mean(1)]).float().contiguous())

    def __call__(self, sources, estimates, lengths=None) -> list[dict[str, float]]:
        """One dict per mixture, {"SI-SDR", "SNR"}: the means over the mixture's estimates.  Rows at the
        metric's ``sample_rate``; ``lengths``: [B] ints, one per mixture."""
        return self.compute_metric(sources, estimates, lengths)
