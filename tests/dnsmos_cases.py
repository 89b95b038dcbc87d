"""The fixtures and bars of tests/test_dnsmos_cpu.py and tests/test_dnsmos_gpu.py.

The fixtures (tests/golden/dnsmos_*.npz, written by tests/golden/make_dnsmos_golden.py) hold the
reference's own DNSMOS results on stored rows:

    ref32    the reference's code in float32 -- what both modes are compared with
    ref16    the reference as it is (half-precision autocast), NaN on quiet rows -- documentation
    mixed16  float32 front end, the reference's layers under CPU float16 autocast -- the engine's arithmetic
    basis, basis_raw = max |mixed16 - ref32| over the fixture's rows and keys (scores, raw outputs)

Bars.  CPU mode: 1e-4 MOS from ref32 (about 30 times the float32-against-float64 gap of the network,
3e-6; far below the 1e-3 differences between rows).  Engine: twice the fixture's stored basis (MFMA
accumulation order differs from the CPU f16 kernels' while the rounding per layer is the same size);
the scores against ``basis``, the per-segment raw outputs against ``basis_raw``.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
WEIGHTS = os.path.join(GOLDEN, "dnsmos_sig_bak_ovr.npz")
FIXTURES = ("dnsmos_16k", "dnsmos_short", "dnsmos_long", "dnsmos_8k")
CPU_BAR = 1e-4
SEG, HOP = 144160, 16000
# lengths of the segment-count checks, and the expected counts of some of them
SEGMENT_LENGTHS = (1, 319, 320, 40000, 72079, 72080, 144159, 144160, 144161, 160159, 160160, 176160)
KNOWN_SEGMENTS = {144159: 10, 144160: 1, 160160: 2, 40000: 1, 177000: 3}


def segments_rule(n: int) -> int:
    """The reference's segment count (DNSMOS.py:113-116), by its doubling loop."""
    if n < 1:
        return 0
    while n < SEG:
        n += n
    return len(range(0, n - SEG + 1, HOP))


class Fixture:
    def __init__(self, name: str):
        with np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False) as z:
            self.name = name
            self.sample_rate = int(z["sample_rate"])
            self.rows = torch.from_numpy(z["noisy"].astype(np.float32) / 32768.0) * torch.from_numpy(z["scale"])[:, None]
            self.ref32, self.ref32_raw = z["ref32"], z["ref32_raw"]
            self.ref16 = z["ref16"]
            self.mixed16 = z["mixed16"]
            self.basis, self.basis_raw = float(z["basis"]), float(z["basis_raw"])


_cache = {}


def fixture(name: str) -> Fixture:
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def _np(x):
    if isinstance(x, list):
        x = [[r["SIG"], r["BAK"], r["OVRL"]] for r in x]
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def assert_within(got, want, bar: float, what: str):
    """|got - want| <= bar everywhere, every value finite; prints the worst deviation first."""
    g, w = _np(got), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    err = np.abs(g - w)
    print(f"{what}: worst |got - expected| = {np.nanmax(err):.3e} (bar {bar:.3e})")
    assert np.isfinite(g).all(), (what, g)
    assert (err <= bar).all(), (what, g, w, err)


def features64(weights: dict, rows: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[S_total, 900, 161] log-power images of full-length rows of at least 144160 samples, from the
    checkpoint's two matrices, in ``dtype`` on the CPU."""
    wr = weights["conv_real_stft.weight"].reshape(161, 320).to(dtype)
    wi = weights["conv_imag_stft.weight"].reshape(161, 320).to(dtype)
    out = []
    for row in rows:
        fr = row.to(dtype).unfold(0, SEG, HOP).unfold(1, 320, 160)
        re, im = fr @ wr.T, fr @ wi.T
        out.append(torch.log10(torch.clamp_min(re.square() + im.square(), 1e-12)))
    return torch.cat(out)
