"""The references, the error measure and the bars of tests/test_dnsmos_grad_cpu.py and tests/test_dnsmos_grad_gpu.py.

Two statements of the gradient of the DNSMOS scores with respect to a row's samples, both torch autograd through
the package's own ``_cpu.dnsmos_features`` and the network, in float64 on the CPU:

    float64     ``_cpu.dnsmos_network`` as it is -- what the engine is compared with
    emulation   the same graph carrying the engine's forward roundings (``emulated_network``): the image rounded
                to float32, conv2 ... conv7's weights rounded to f16, every stored activation rounded to f16 after
                ReLU (and pool).  ``Round`` rounds the value forward and passes the gradient through unchanged, so
                the emulation's gradient is exact arithmetic on the rounded forward's decisions.

Error measure (``deviation``): the largest absolute deviation over the row's largest absolute float64 gradient
element.  The bar of the engine is twice the emulation's own deviation from float64 (``basis`` and, for the image
gradient alone, ``basis_image`` of tests/golden/dnsmos_grad_basis.json, written by
tests/golden/make_dnsmos_grad_golden.py): the engine rounds as the emulation does, MFMA accumulation order
differs from the emulation's and moves near-tie decisions -- tests/dnsmos_cases.py's rule for the scores.
"""
import functools
import json
import os

import numpy as np
import torch

from fast_speech_enhancement_metrics_amd import _cpu
from fast_speech_enhancement_metrics_amd.DNSMOS import load_weights

from . import dnsmos_cases as dc

BASIS_FILE = os.path.join(dc.GOLDEN, "dnsmos_grad_basis.json")
MARGIN = 2.0
MIXED = (0.5, -1.0, 2.0)   # an upstream gradient over (SIG, BAK, OVRL)
SEG, HOP = dc.SEG, dc.HOP


@functools.lru_cache(maxsize=None)
def weights():
    return load_weights(dc.WEIGHTS)


@functools.lru_cache(maxsize=None)
def weights64():
    return {k: v.to(torch.float64) for k, v in weights().items()}


@functools.lru_cache(maxsize=None)
def basis():
    """{"basis": ..., "basis_image": ...} as recorded."""
    with open(BASIS_FILE) as f:
        return json.load(f)


def poly64():
    """The polynomial's float32 constants (the engine's) as float64 tensors."""
    return tuple(torch.tensor(c, dtype=torch.float32).to(torch.float64) for c in _cpu._DNSMOS_POLY)


class Round(torch.autograd.Function):
    """x rounded to ``dtype`` and back; the gradient passes unchanged."""

    @staticmethod
    def forward(ctx, x, dtype):
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def emulated_network(w: dict, image: torch.Tensor) -> torch.Tensor:
    """``_cpu.dnsmos_network`` in the image's dtype with the engine's forward roundings."""
    F = torch.nn.functional
    h = Round.apply(image, torch.float32).unsqueeze(1)
    for i in (0, 2, 4, 6, 9, 12, 15):
        wt = w[f"conv_layers.{i}.weight"]
        if i != 0:   # (conv1 runs in float32 from float32 weights)
            wt = wt.to(torch.float16).to(wt.dtype)
        h = F.relu(F.conv2d(h, wt, w[f"conv_layers.{i}.bias"], padding=1))
        if i in _cpu._DNSMOS_POOL_AFTER:
            h = F.max_pool2d(h, 2)
        if i != 15:   # (conv7's output is not stored: its maxima stay float32)
            h = Round.apply(h, torch.float16)
    h = h.amax(dim=(2, 3))
    h = F.relu(F.linear(h, w["output_layers.0.weight"], w["output_layers.0.bias"]))
    h = F.relu(F.linear(h, w["output_layers.2.weight"], w["output_layers.2.bias"]))
    return F.linear(h, w["output_layers.4.weight"], w["output_layers.4.bias"])


def segments64(x: torch.Tensor) -> torch.Tensor:
    """[S, 144160] float64 segments of a 1-D row on its graph (periodic continuation)."""
    n = x.numel()
    m = n
    while m < SEG:
        m *= 2
    return x.to(torch.float64).repeat(m // n).unfold(0, SEG, HOP)


def scores64(row: torch.Tensor, network=_cpu.dnsmos_network) -> torch.Tensor:
    """[3] float64 scores of a 1-D row on its graph, the directly composed statement."""
    c0, c1, c2 = poly64()
    segs = segments64(row)
    raw = torch.cat([network(weights64(), _cpu.dnsmos_features(weights64(), segs[s:s + 1], dtype=torch.float64))
                     for s in range(segs.shape[0])])
    return (c0 + c1 * raw + c2 * raw.square()).mean(0)


def gradients(row: torch.Tensor, network=_cpu.dnsmos_network, keys=(0, 1, 2), images=False):
    """(scores [3], d score_k / d row [len(keys), n]) float64 numpy of a 1-D row, segment by segment; with
    ``images`` also d score_k / d image [len(keys), S, 900, 161]."""
    c0, c1, c2 = poly64()
    x = row.to(torch.float64).clone().requires_grad_(True)
    segs = segments64(x)
    S = segs.shape[0]
    scores = torch.zeros(3, dtype=torch.float64)
    grads = torch.zeros(len(keys), x.numel(), dtype=torch.float64)
    gimg = torch.zeros(len(keys), S, 900, 161, dtype=torch.float64)
    for s in range(S):
        image = _cpu.dnsmos_features(weights64(), segs[s:s + 1], dtype=torch.float64)
        raw = network(weights64(), image)
        poly = (c0 + c1 * raw + c2 * raw.square())[0] / S
        scores += poly.detach()
        for j, k in enumerate(keys):
            g, gi = torch.autograd.grad(poly[k], (x, image), retain_graph=j + 1 < len(keys))
            grads[j] += g
            gimg[j, s] = gi[0]
    out = (scores.numpy(), grads.numpy())
    return out + (gimg.numpy(),) if images else out


def image_gradients(image: torch.Tensor, network=_cpu.dnsmos_network, keys=(0, 1, 2)):
    """d score_k / d image [len(keys), 900, 161] float64 numpy of one segment's image [900, 161]."""
    c0, c1, c2 = poly64()
    im = image.to(torch.float64).clone()[None].requires_grad_(True)
    raw = network(weights64(), im)
    poly = (c0 + c1 * raw + c2 * raw.square())[0]
    return np.stack([torch.autograd.grad(poly[k], im, retain_graph=j + 1 < len(keys))[0][0].numpy()
                     for j, k in enumerate(keys)])


def deviation(got, want) -> float:
    """The largest absolute deviation over the largest absolute element of ``want`` (float64)."""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    return float(np.abs(g - w).max() / np.abs(w).max())


@functools.lru_cache(maxsize=None)
def reference(name: str, b: int, keys=(0, 1, 2)):
    """``gradients`` of row b of a fixture of tests/dnsmos_cases.py, computed once."""
    return gradients(dc.fixture(name).rows[b], keys=keys)
