"""DNSMOS metric -- drop-in for the reference's ``fast_se_metrics.DNSMOS`` (DNSMOS.py:86-136): SIG, BAK
and OVRL, a no-reference MOS estimate from the SIG_BAK_OVR network.

Rows are scored at 16 kHz (other rates go through the package's resampler): a row is continued
periodically to at least 9.01 s, cut into 144160-sample segments every 16000 samples, each segment
becomes a 900 x 161 log-power image, seven 3 x 3 convolutions and three dense layers give three raw
outputs, a polynomial maps them to MOS, and the row's scores are the means over its segments
(include/fsem_dnsmos.h).  ``use_gpu=True``: the engine (``fsem_dnsmos_f32``, csrc/dnsmos.hip, in
libfsem_dnsmos.so: f16 MFMA convolutions, float32 front end); ``use_gpu=False``: the package's CPU
implementation (``_cpu.dnsmos``, float32 torch ops).

Two deviations from the reference: the log-power image is float32 (the reference's half-precision
autocast turns quiet bins into -inf and the row's scores into NaN; here they are finite), and a row of
no samples scores NaN (the reference never returns on it).

``clean`` is not used: ``metric(None, denoised)`` and ``metric(clean, denoised)`` give the same scores;
a ``clean`` of another shape raises the reference's exception.

``differentiable_scores`` and ``loss`` are the same scores with the gradient with respect to the rows
(include/fsem.h, "DNSMOS with gradients"): on the engine ``fsem_dnsmos_f32``
forward, which keeps nothing, and ``fsem_dnsmos_grad_f32`` backward (csrc/dnsmos_grad.hip, in libfsem.so),
which recomputes each pass of segments and runs the adjoint on f16 MFMA; in CPU mode ``_cpu.dnsmos_features``
and ``_cpu.dnsmos_network`` in float64 under torch's own autograd.

Weights: ``weights=`` names an ``.npz`` of the checkpoint's 22 tensors as float32 arrays under their
state-dict names (tests/golden/dnsmos_sig_bak_ovr.npz; tensors it lacks are read from the file
``<name>_2.npz`` beside it) or a state-dict ``.pt`` (loaded with ``weights_only=True``).  None: the
file named by the environment variable FSEM_DNSMOS_WEIGHTS, else tests/golden/dnsmos_sig_bak_ovr.npz
of the source tree this package lies in.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _cpu, _native
from .base import (BaseMetric, as_rows, check_row_rate, device_lengths, grad_buffer, noisy_shape, resample_rows,
                   scored_mean)

_PKG = os.path.dirname(os.path.abspath(__file__))
DEFAULT_WEIGHTS = os.path.join(_PKG, "..", "tests", "golden", "dnsmos_sig_bak_ovr.npz")
_CONVS = (("conv_layers.0", 128, 1), ("conv_layers.2", 64, 128), ("conv_layers.4", 64, 64), ("conv_layers.6", 32, 64),
          ("conv_layers.9", 32, 32), ("conv_layers.12", 32, 32), ("conv_layers.15", 64, 32))
_DENSE = (("output_layers.0", 128, 64), ("output_layers.2", 64, 128), ("output_layers.4", 3, 64))
# the 22 tensors in state-dict order (the order fsem_dnsmos_pack_weights_f32 takes them in) and their shapes
WEIGHT_SHAPES = {"conv_real_stft.weight": (161, 320, 1), "conv_imag_stft.weight": (161, 320, 1)}
for _n, _o, _i in _CONVS:
    WEIGHT_SHAPES[_n + ".weight"] = (_o, _i, 3, 3)
    WEIGHT_SHAPES[_n + ".bias"] = (_o,)
for _n, _o, _i in _DENSE:
    WEIGHT_SHAPES[_n + ".weight"] = (_o, _i)
    WEIGHT_SHAPES[_n + ".bias"] = (_o,)
assert len(WEIGHT_SHAPES) == _native.DNSMOS_NUM_TENSORS


def weights_path(weights=None) -> str:
    """The weights file: ``weights``, else FSEM_DNSMOS_WEIGHTS, else the tree's fixture; raises
    FileNotFoundError (naming both options) if it does not exist."""
    path = weights if weights is not None else os.environ.get("FSEM_DNSMOS_WEIGHTS") or DEFAULT_WEIGHTS
    path = os.path.abspath(os.fspath(path))
    if not os.path.isfile(path):
        raise FileNotFoundError(
            f"DNSMOS weights not found: {path}.  Pass weights= (an .npz of the checkpoint's 22 float32 tensors under "
            "their state-dict names, or a state-dict .pt) or set FSEM_DNSMOS_WEIGHTS to such a file; the default is "
            "tests/golden/dnsmos_sig_bak_ovr.npz of the source tree.")
    return path


def load_weights(path: str) -> dict:
    """{state-dict name: float32 CPU tensor} of the 22 tensors, shapes checked."""
    if path.endswith(".npz"):
        import numpy as np
        arrays = {}
        second = path[:-4] + "_2.npz"
        for p in (path, second) if os.path.isfile(second) else (path,):
            with np.load(p, allow_pickle=False) as z:
                arrays.update({k: z[k] for k in z.files})
        sd = {k: torch.from_numpy(v) for k, v in arrays.items()}
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    out = {}
    for name, shape in WEIGHT_SHAPES.items():
        if name not in sd:
            raise ValueError(f"DNSMOS weights {path}: tensor {name} is missing")
        t = torch.as_tensor(sd[name]).detach().to("cpu", torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"DNSMOS weights {path}: {name} has shape {tuple(t.shape)}, expected {shape}")
        out[name] = t
    return out


class _EngineScores(torch.autograd.Function):
    """scores [B, 3] float32 of CUDA rows [B, L] at rate ``sr`` by the engine, bitwise ``scores`` (the same call,
    after the resampler for other rates); nothing is kept but the 16 kHz rows.  The backward is
    fsem_dnsmos_grad_f32, which recomputes the forward pass by pass, and, for other rates, the transposed
    resampler (fsem_resample_rows_grad_f32) behind it: the gradient is taken at the float32 16 kHz rows the
    scores were taken at."""

    @staticmethod
    def forward(ctx, rows, lens, sr, metric):
        ctx.shape, ctx.sr, ctx.lens, ctx.metric = tuple(rows.shape), sr, lens, metric
        if sr != metric.EXPECTED_SAMPLING_RATE:  # (scores(): the forward resampler's float32 rows)
            rows, lens = metric._engine_rows(rows, sr, lens)
        ctx.rows = (rows, lens)
        return metric._rows_scores(rows, metric.EXPECTED_SAMPLING_RATE, lens)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_scores):
        B, L = ctx.shape
        rows, lens = ctx.rows
        L16 = rows.shape[1]
        at_rate = ctx.sr != 16000
        lib = _native.load()
        # (the 16 kHz gradient: the caller's buffer, or one as wide as the transposed resampler reads)
        width = max(L16, int(lib.fsem_resample_length(L, ctx.sr, 16000))) if at_rate else L16
        grad, g = grad_buffer((B, L16, width), L16 > 0, (g_scores,))
        if g is None:
            return grad.new_zeros(B, L), None, None, None
        segments = int(_native.load_dnsmos().fsem_dnsmos_segments(L16))
        P = min(_native.DNSMOS_MAX_PASS, B * (max(segments, 10) if lens is not None else segments))
        scratch = _native.workspace(4 * lib.fsem_dnsmos_grad_scratch_floats(B, L16, P), rows.device)
        blob = ctx.metric.grad_blob(rows.device)
        stream = _native.stream_handle(rows.device)
        rc = lib.fsem_dnsmos_grad_f32(rows.data_ptr(), B, L16, rows.stride(0), _native.ptr(lens), blob.data_ptr(),
                                      g[0].data_ptr(), grad.data_ptr(), grad.stride(0), None, scratch.data_ptr(), P,
                                      stream)
        _native.check(rc, "DNSMOS backward")
        if at_rate:
            grad16, (grad, _) = grad, grad_buffer((B, L, L), True, (g_scores,))
            rc = lib.fsem_resample_rows_grad_f32(grad16.data_ptr(), B, L, grad16.stride(0), _native.ptr(ctx.lens),
                                                 grad.data_ptr(), grad.stride(0), ctx.sr, 16000, stream)
            _native.check(rc, "DNSMOS backward")
        return grad, None, None, None


class DNSMOS(BaseMetric):
    higher_is_better = True
    EXPECTED_SAMPLING_RATE = 16000
    KEYS = ("SIG", "BAK", "OVRL")
    _TRANSIENT = BaseMetric._TRANSIENT + ("_blobs",)

    def __init__(self, sample_rate: int = 16000, use_gpu: bool = False, *, devices=None, weights=None):
        super().__init__(sample_rate, use_gpu, devices=devices)
        self.weights_file = weights_path(weights)  # (a missing file raises here, not at the first call)
        self.weights = load_weights(self.weights_file)
        if use_gpu:
            _native.load_dnsmos()  # (a missing engine raises here too)
        self._blobs = {}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._blobs = {}

    def blob(self, device) -> torch.Tensor:
        """The engine's packed weights on ``device`` (fsem_dnsmos_pack_weights_f32), built once per device."""
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        blob = self._blobs.get(idx)
        if blob is None:
            lib = _native.load_dnsmos()
            with torch.cuda.device(idx):
                dev = [self.weights[k].to(torch.device("cuda", idx)) for k in WEIGHT_SHAPES]
                ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
                blob = torch.empty(lib.fsem_dnsmos_weights_bytes(), dtype=torch.uint8, device=dev[0].device)
                rc = lib.fsem_dnsmos_pack_weights_f32(ptrs, blob.data_ptr(), blob.numel(),
                                                      _native.stream_handle(blob.device))
                _native.check(rc, "DNSMOS weights")
                # once per device: the blob is complete before any stream reads it (and before the
                # float32 copies are freed)
                torch.cuda.current_stream(blob.device).synchronize()
            self._blobs[idx] = blob
        return blob

    def grad_blob(self, device) -> torch.Tensor:
        """The backward's packed weights on ``device`` (fsem_dnsmos_grad_pack_weights_f32), built once per device
        and kept beside the forward's."""
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        blob = self._blobs.get(("grad", idx))
        if blob is None:
            lib = _native.load()
            with torch.cuda.device(idx):
                dev = [self.weights[k].to(torch.device("cuda", idx)) for k in WEIGHT_SHAPES]
                ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
                blob = torch.empty(lib.fsem_dnsmos_grad_weights_floats(), dtype=torch.float32, device=dev[0].device)
                rc = lib.fsem_dnsmos_grad_pack_weights_f32(ptrs, blob.data_ptr(), blob.numel(),
                                                           _native.stream_handle(blob.device))
                _native.check(rc, "DNSMOS gradient weights")
                torch.cuda.current_stream(blob.device).synchronize()  # (as blob())
            self._blobs[("grad", idx)] = blob
        return blob

    def scores(self, denoised_speech, sample_rate: int | None = None, lengths=None) -> torch.Tensor:
        """[B, 3] float32 (SIG, BAK, OVRL) on the metric's device, without a host sync.

        Rows at ``sample_rate``; None means rows already at 16 kHz, which requires a 16 kHz metric.
        Other rates are resampled to 16 kHz first, each row as the row alone.  ``lengths`` (optional,
        [B] ints at that rate): row b holds lengths[b] samples and scores as the unpadded row alone would.
        """
        sr = check_row_rate(self, sample_rate)
        if self.fans_out():
            cols = self.fan_out(lambda c, n, lk: tuple(self._rows_scores(n, sr, lk).unbind(1)), denoised_speech,
                                denoised_speech, lengths, 3, balance=lengths)
            return torch.stack(cols, dim=1)
        return self._rows_scores(denoised_speech, sr, lengths)

    def _engine_rows(self, denoised_speech, sr: int, lengths):
        """(rows [B, L] float32, lengths int32 on the rows' device | None) at 16 kHz."""
        if sr != self.EXPECTED_SAMPLING_RATE:
            _, denoised_speech, lengths = resample_rows(None, denoised_speech, lengths, sr, self.EXPECTED_SAMPLING_RATE)
        rows = as_rows(denoised_speech)
        B, L = rows.shape
        lens = device_lengths(lengths, B, L, rows.device) if lengths is not None else None
        return rows, lens

    def _rows_scores(self, denoised_speech, sr: int, lengths) -> torch.Tensor:
        """scores [B, 3] of rows at rate ``sr`` on their own device (one engine call)."""
        rows, lens = self._engine_rows(denoised_speech, sr, lengths)
        B, L = rows.shape
        if not rows.is_cuda:
            return _cpu.dnsmos(self.weights, rows, lens)
        out = torch.empty(B, 3, dtype=torch.float32, device=rows.device)
        if B == 0:
            return out
        if L == 0:  # (the engine takes rows of at least one sample: a row of no samples is NaN)
            return out.fill_(float("nan"))
        lib = _native.load_dnsmos()
        blob = self.blob(rows.device)
        ws = _native.workspace(lib.fsem_dnsmos_workspace_bytes(B, L), rows.device)
        rc = lib.fsem_dnsmos_f32(rows.data_ptr(), B, L, rows.stride(0), _native.ptr(lens),
                                 blob.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _native.stream_handle(rows.device))
        _native.check(rc, "DNSMOS")
        return out

    # ------------------------------------------------------------------ scores to train against
    def differentiable_scores(self, denoised_speech: torch.Tensor, sample_rate: int | None = None,
                              lengths=None) -> torch.Tensor:
        """[B, 3] (SIG, BAK, OVRL) as ``scores``, carrying the gradient with respect to ``denoised_speech``:
        float32 and bitwise ``scores()`` on the engine, float64 in CPU mode.  On the engine the gradient is that
        of the f16 forward the scores come from (its ReLU, pool and maximum decisions; INTEGRATION.md section 20
        gives the measured distance to the float64 gradient).  A row that scores NaN gets a zero gradient row.
        Rows at another rate are resampled as ``scores`` resamples them, to float32 16 kHz rows, and the gradient
        at those rows is pulled back through the transposed resampler (``fsem_resample_rows_grad_f32``)."""
        if self._fanout is not None:
            raise NotImplementedError("DNSMOS: devices= is not supported with gradients (the multi-device fan-out "
                                      "returns detached scores)")
        sr = check_row_rate(self, sample_rate)
        noisy = torch.atleast_2d(torch.as_tensor(denoised_speech))
        if noisy.dim() != 2:
            noisy = noisy.reshape(-1, noisy.shape[-1])
        if not noisy.is_cuda:
            return self._differentiable_cpu(noisy, sr, lengths)
        rows = noisy.to(torch.float32)  # (autograd casts the gradient back)
        if rows.stride(-1) != 1 or rows.stride(0) < rows.shape[1]:
            rows = rows.contiguous()
        B, L = rows.shape
        if B == 0 or L == 0:  # no rows, or rows of no samples: the scores, and an empty gradient
            return self._rows_scores(rows.detach(), sr, lengths) + rows.sum(1, keepdim=True) * 0
        lens = device_lengths(lengths, B, L, rows.device) if lengths is not None else None
        return _EngineScores.apply(rows, lens, sr, self)

    def _differentiable_cpu(self, noisy, sr: int, lengths) -> torch.Tensor:
        B, L = noisy.shape
        lens = device_lengths(lengths, B, L, "cpu").tolist() if lengths is not None else [L] * B
        w64 = {k: v.to(torch.float64) for k, v in self.weights.items()}
        c0, c1, c2 = (torch.tensor(c, dtype=torch.float32).to(torch.float64) for c in _cpu._DNSMOS_POLY)
        out = []
        for b in range(B):  # (a plain loop: each row's graph hangs on its own slice of `noisy`)
            n = int(lens[b])
            row = noisy[b, :n]
            if sr != self.EXPECTED_SAMPLING_RATE and n > 0:
                # the value at the float32 rows scores() resamples, the derivative the resampler's in float64
                _, at, _ = resample_rows(None, row.detach()[None], None, sr, self.EXPECTED_SAMPLING_RATE)
                y = _cpu.resample64(row[None], sr, self.EXPECTED_SAMPLING_RATE)
                row = (at.to(torch.float64) + (y - y.detach()))[0]
                n = row.numel()
            S = _cpu.dnsmos_segments(n)
            used = n if n <= _cpu.DNSMOS_SEGMENT else _cpu.DNSMOS_HOP * (S - 1) + _cpu.DNSMOS_SEGMENT
            if n < 1 or not bool(torch.isfinite(row.detach()[:used]).all()):
                out.append(torch.full((1, 3), float("nan"), dtype=torch.float64))
                continue
            m = n
            while m < _cpu.DNSMOS_SEGMENT:
                m *= 2
            segs = row.to(torch.float64).repeat(m // n).unfold(0, _cpu.DNSMOS_SEGMENT, _cpu.DNSMOS_HOP)
            raw = torch.cat([_cpu.dnsmos_network(w64, _cpu.dnsmos_features(w64, segs[i:i + 2], dtype=torch.float64))
                             for i in range(0, S, 2)])
            out.append((c0 + c1 * raw + c2 * raw.square()).mean(0, keepdim=True))
        return torch.cat(out) if B else torch.zeros(0, 3, dtype=torch.float64)

    def loss(self, denoised_speech: torch.Tensor, sample_rate: int | None = None, lengths=None,
             key: str = "OVRL") -> torch.Tensor:
        """-mean of ``key`` (one of KEYS; higher is better) over the rows with a finite score: a scalar that
        carries the gradient with respect to ``denoised_speech``.  With no such row: a zero with a zero gradient."""
        if key not in self.KEYS:
            raise ValueError(f"DNSMOS.loss: key must be one of {self.KEYS}, got {key!r}")
        score = self.differentiable_scores(denoised_speech, sample_rate, lengths)[:, self.KEYS.index(key)]
        mean, _ = scored_mean(score, torch.isfinite(score.detach()), denoised_speech)
        return -mean

    def compute_metric(self, clean_speech: torch.Tensor | None, denoised_speech: torch.Tensor,
                       lengths=None) -> list[dict[str, float]]:
        if clean_speech is not None and noisy_shape(clean_speech) != noisy_shape(denoised_speech):
            raise Exception("`clean_speech` and `denoised_speech` should have the same shape.")
        with torch.no_grad():
            s = self.scores(denoised_speech, self.EXPECTED_SAMPLING_RATE, lengths=lengths)
            return self.result_list(s.float().t().contiguous())  # [3, B]
