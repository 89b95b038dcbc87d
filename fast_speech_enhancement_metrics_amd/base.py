"""BaseMetric -- the reference's drop-in boundary (fast_se_metrics/base.py:6-43), unchanged API.

``metric = PESQ(sample_rate, use_gpu)`` then ``metric(clean, denoised) -> list[dict]``.
``use_gpu=True`` runs the gfx950 HIP engine (libfsem); it raises at construction if the
engine is missing -- there is no silent fallback.  ``use_gpu=False`` runs the package's
own CPU implementation (``_cpu.py``), the reference's CPU mode.
"""
from __future__ import annotations

import functools
from abc import ABC, abstractmethod

import torch

from . import _native
from .batching import as_lengths, pad_batch, resampled_lengths
from .resample import Resample


class BaseMetric(ABC):
    higher_is_better: bool
    EXPECTED_SAMPLING_RATE: int

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, devices=None):
        """``devices`` (extension; GPU only): None = the current device, as the reference; ``"all"``,
        a count, or a list of devices (repeats allowed) = each call's rows split over those
        devices from this one process (multidevice.py), scores returned on the first."""
        self.sample_rate = sample_rate
        self.device = "cuda" if use_gpu else "cpu"
        self.resampler = Resample(sample_rate, self.EXPECTED_SAMPLING_RATE)
        self.resampler.to(self.device)
        self.devices = None
        self._fanout = None
        if use_gpu:
            if not torch.cuda.is_available():
                raise RuntimeError("use_gpu=True but no HIP device is visible")
            _native.load()
            from .multidevice import FanOut, resolve_devices
            self.devices = resolve_devices(devices)
            if self.devices is not None:  # (one listed device: its own thread and stream alike)
                self._fanout = FanOut(self.devices)

    # ---- what a GPU metric keeps between calls (the drop-in call's pinned score buffers and
    # event per host thread and device, the last result list's fill handle, the fan-out's
    # threads and streams) is process state: it is dropped when a metric is copied or pickled
    # (the reference's BaseMetric is a plain object; copies of it stay possible) and rebuilt on use.
    _TRANSIENT = ("_fsem_tls", "_held_list", "_fanout")

    def release(self) -> None:
        """Free the pinned score buffers and the last result list this metric keeps for its next
        call (they are rebuilt on the next call)."""
        _native.release(self)

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in self._TRANSIENT:
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._fanout = None
        if self.devices is not None:
            from .multidevice import FanOut
            self._fanout = FanOut(self.devices)

    def home_device(self):
        """Where results live: the first listed device of a multi-device metric, else ``.device``."""
        return self.device if self.devices is None else self.devices[0]

    def fan_out(self, score, clean, noisy, lengths, ncols: int, balance=None):
        """``score(clean_rows, noisy_rows, lengths_rows)`` over this metric's devices (multidevice.py)
        -> ncols [B] float32 tensors on the first listed device."""
        return self._fanout.run(score, torch.atleast_2d(clean), torch.atleast_2d(noisy), lengths, ncols,
                                balance_lengths=balance)

    def fans_out(self) -> bool:
        """This call's rows go to several devices (a multi-device metric, not already on a shard)."""
        if self._fanout is None:
            return False
        from .multidevice import in_shard
        return not in_shard()

    def prepare_audio(self, audio: torch.Tensor, lengths: torch.Tensor | None = None) -> torch.Tensor:
        """The reference's prepare_audio (base.py:16-21); with ``lengths`` each row is resampled as
        its unpadded self (Resample.forward).  A multi-device metric leaves rows at the expected
        rate where they are: each shard copies its own rows to its device."""
        audio = torch.atleast_2d(audio)
        if self.fans_out() and self.sample_rate == self.EXPECTED_SAMPLING_RATE:
            return audio
        home = self.home_device()
        audio = audio.to(home)
        if self.sample_rate != self.EXPECTED_SAMPLING_RATE:
            if self.devices is not None:
                # the engine launches on the current HIP device (include/fsem.h): make the home
                # device current while its stream resamples (devices=[1, ...] called with 0 current)
                with torch.cuda.device(home):
                    audio = self.resampler(audio, lengths)
            else:
                audio = self.resampler(audio, lengths)
        return audio

    def prepare_inputs(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths: torch.Tensor | None = None):
        if clean_speech is not None and clean_speech.shape != denoised_speech.shape:
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        if clean_speech is not None:
            clean_speech = self.prepare_audio(clean_speech, lengths)
        denoised_speech = self.prepare_audio(denoised_speech, lengths)
        return clean_speech, denoised_speech

    def result_list(self, t: torch.Tensor) -> list[dict[str, float]]:
        """The drop-in call's result, a dict over ``self.KEYS`` per row, from [K, B] float32 scores."""
        if t.is_cuda:  # the dicts are built while the GPU computes, then filled
            return _native.list_from_device(self, t, self.KEYS)[0]
        return _native.score_list(t, self.KEYS)

    @abstractmethod
    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths: torch.Tensor | None = None) -> list[dict[str, float]]:
        raise NotImplementedError

    def __call__(self, clean_speech, denoised_speech, lengths=None) -> list[dict[str, float]]:
        """The reference's call (base.py:41-43), extended to ragged batches: lists of 1-D
        utterances, or padded [B, L] tensors with per-row ``lengths`` (see batching.py)."""
        clean_speech, denoised_speech, lengths = self.split_ragged(clean_speech, denoised_speech, lengths)
        # with lengths, the resampler sees each row as the row alone would be (zeros past it)
        clean_speech, denoised_speech = self.prepare_inputs(clean_speech, denoised_speech, lengths)
        if lengths is None:
            return self.compute_metric(clean_speech, denoised_speech)
        lengths = resampled_lengths(lengths, self.sample_rate, self.EXPECTED_SAMPLING_RATE)
        return self.compute_metric(clean_speech, denoised_speech, lengths=lengths)

    @staticmethod
    def split_ragged(clean_speech, denoised_speech, lengths):
        """-> (clean, denoised, lengths | None) with lengths validated against the row capacity."""
        if isinstance(denoised_speech, (list, tuple)):
            if lengths is not None:
                raise ValueError("pass either lists of utterances or padded tensors with lengths")
            return pad_batch(clean_speech, denoised_speech)
        if lengths is not None:
            d = torch.atleast_2d(denoised_speech)
            lengths = as_lengths(lengths, d.shape[0], d.shape[-1])
        return clean_speech, denoised_speech, lengths


def zero_tail(x: torch.Tensor | None, lengths: torch.Tensor) -> torch.Tensor | None:
    """Zero every sample of row b at or past lengths[b]."""
    if x is None:
        return None
    x = torch.atleast_2d(x)
    t = torch.arange(x.shape[-1], device=x.device)
    return torch.where(t[None, :] < lengths.to(x.device, torch.int64)[:, None], x, torch.zeros((), dtype=x.dtype,
                                                                                               device=x.device))


def device_lengths(lengths, batch: int, capacity: int, device) -> torch.Tensor:
    """Validated int32 per-row lengths on `device` (the C-ABI's `lengths` array)."""
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda and lengths.dtype == torch.int32 \
            and lengths.numel() == batch and lengths.device == torch.device(device):
        # trusted device array on the rows' device: no host round trip (the kernels clamp each
        # length to [0, L])
        return lengths.contiguous()
    return as_lengths(lengths, batch, capacity).to(device)


def same_device(clean: torch.Tensor, noisy: torch.Tensor) -> None:
    """The engine reads both operands on one device, as torch's own ops in the reference require
    (a host pointer handed to a kernel would fault the GPU instead of raising)."""
    if clean.device != noisy.device:
        raise RuntimeError("Expected all tensors to be on the same device, but found at least two devices, "
                           f"{clean.device} and {noisy.device}!")


def as_rows(x: torch.Tensor) -> torch.Tensor:
    """float32 [B, L] with unit stride along time (row stride = x.stride(0))."""
    x = torch.atleast_2d(x)
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.dim() != 2 or x.stride(-1) != 1 or x.stride(0) < x.shape[1]:
        x = x.reshape(-1, x.shape[-1]).contiguous()
    return x


def pair_rows(clean, noisy):
    """(clean, noisy) as float32 [B, L] rows (as_rows) of one shape on one device."""
    clean = as_rows(clean)
    noisy = as_rows(noisy)
    if noisy.shape != clean.shape:
        raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
    same_device(clean, noisy)
    return clean, noisy


def engine_rows(clean: torch.Tensor, noisy: torch.Tensor, lengths, *, empty_as_zeros: bool = False,
                aligned16: bool = False):
    """pair_rows' CUDA rows as an engine call takes them: (clean, noisy, L, lens) with one row
    stride, every row readable up to ceil4(L) floats (include/fsem.h) and ``lengths`` validated
    against the rows as given, as an int32 device array or None.

    ``empty_as_zeros``: rows of no samples (L == 0) become four zero samples with zero lengths, for
    the engines that score such rows; otherwise L == 0 comes back and the caller does not launch.
    ``aligned16``: the row stride a multiple of 4 floats and both bases 16-byte aligned as well,
    for an engine that reads rows in 16-byte pieces (Composite's PESQ stage)."""
    B, L = clean.shape
    lens = device_lengths(lengths, B, L, clean.device) if lengths is not None else None
    if L == 0 and empty_as_zeros:
        clean, noisy, L = clean.new_zeros(B, 4), noisy.new_zeros(B, 4), 4
        lens = torch.zeros(B, dtype=torch.int32, device=clean.device)
    if clean.stride(0) != noisy.stride(0) or L % 4 or \
            (aligned16 and (clean.stride(0) % 4 or (clean.data_ptr() | noisy.data_ptr()) % 16)):
        pad = (-L) % 4
        clean = torch.nn.functional.pad(clean, (0, pad)).contiguous()
        noisy = torch.nn.functional.pad(noisy, (0, pad)).contiguous()
    return clean, noisy, L, lens


# ---- the scores to train against (STOI.loss, PESQ.loss): what their host paths share

def grad_operands(metric, clean_speech, denoised_speech):
    """(clean.detach(), noisy) of a ``differentiable_scores`` / ``loss`` call, 2-D, of one shape, on
    one device; ``noisy`` keeps its dtype, its layout and its graph."""
    clean, noisy = torch.as_tensor(clean_speech), torch.as_tensor(denoised_speech)
    if clean.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{type(metric).__name__}: the clean rows are constants; gradients with respect "
                                  "to `clean_speech` are not supported (detach them)")
    clean, noisy = torch.atleast_2d(clean.detach()), torch.atleast_2d(noisy)
    if noisy.shape != clean.shape or clean.dim() != 2:
        raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
    same_device(clean, noisy)
    return clean, noisy


def grad_engine_rows(clean: torch.Tensor, noisy: torch.Tensor, lengths):
    """grad_operands' CUDA rows as engine_rows gives them, (clean, rows, L, lens), with ``rows`` the
    estimate in float32 on its graph (autograd casts the gradient back, and drops the padding)."""
    rows = noisy.to(torch.float32)
    if rows.stride(-1) != 1 or rows.stride(0) < rows.shape[1]:
        rows = rows.contiguous()
    return engine_rows(as_rows(clean), rows, lengths)


def scored_mean(score: torch.Tensor, scored: torch.Tensor, estimate):
    """(mean of ``score`` [B] over the rows ``scored`` [B] bool marks on its device, their count); with no such row
    the mean is a zero on the graph of ``estimate`` (the estimate as the caller gave it), whose
    gradient is zero."""
    count = int(scored.sum())
    total = torch.where(scored, score, torch.zeros((), dtype=score.dtype, device=score.device)).sum()
    if count == 0:  # (an empty sum of the estimate)
        return total * 0 + torch.as_tensor(estimate).reshape(-1)[:0].sum().to(total), 0
    return total / count, count


def grad_buffer(shape, launched: bool, upstream):
    """What a gradient entry writes and reads, (grad [B, width] float32 with [:, L:] zero -- the entry
    writes [:, :L] --, ``upstream`` as contiguous float32), for ``shape`` = (B, L, width); all of
    ``grad`` zero and no upstream (None) when the forward launched nothing."""
    B, L, width = shape
    dev = upstream[0].device
    if not launched:
        return torch.zeros(B, width, dtype=torch.float32, device=dev), None
    grad = torch.empty(B, width, dtype=torch.float32, device=dev)
    grad[:, L:] = 0
    return grad, [g.to(torch.float32).contiguous() for g in upstream]


def noisy_shape(x) -> tuple:
    return tuple(torch.atleast_2d(torch.as_tensor(x)).shape) if x is not None else ()


def check_row_rate(metric, sample_rate: int | None) -> int:
    """Rate of the rows handed to ``metric.scores``.  None means the metric's expected rate, which
    is only unambiguous when the metric was constructed for that rate: a metric built for another
    rate must be told (otherwise its rows would silently be scored at the wrong rate)."""
    if sample_rate is None:
        if metric.sample_rate != metric.EXPECTED_SAMPLING_RATE:
            raise ValueError(f"{type(metric).__name__}({metric.sample_rate}).scores: pass sample_rate= (the rate of "
                             f"the rows; {metric.EXPECTED_SAMPLING_RATE} if they are already resampled)")
        return int(metric.EXPECTED_SAMPLING_RATE)
    return int(sample_rate)


@functools.lru_cache(maxsize=32)
def _resampler(orig: int, new: int) -> Resample:
    # one module per rate pair, kept on the host: its CUDA path runs in libfsem and never reads the
    # kernel buffer, so no per-call host -> device copy (which would wait for the stream to drain)
    return Resample(orig, new)


def resample_rows(clean, noisy, lengths, orig: int, new: int):
    """(clean, noisy, lengths) resampled orig -> new, each row as the row alone when ``lengths`` is
    given (BaseMetric.prepare_audio, base.py:19-20); lengths become the resampled lengths."""
    rs = _resampler(int(orig), int(new))
    noisy = torch.atleast_2d(noisy)
    lens = None
    if lengths is not None:
        lens = device_lengths(lengths, noisy.shape[0], noisy.shape[-1], noisy.device)
    clean = rs(torch.atleast_2d(clean), lens) if clean is not None else None
    noisy = rs(noisy, lens)
    if lens is not None:
        lens = resampled_lengths(lens, orig, new).to(noisy.device)
    return clean, noisy, lens
