"""Scores on fixed seeded inputs, saved for a bitwise A/B of two builds.

Without ``--metrics``: PESQ_STOI of the library named by FSEM_LIB on one synthetic batch.

    FSEM_LIB=.../var/va.so python tools/probes/ab_bitwise.py gpurun_out/a.npy
    FSEM_LIB=.../var/vb.so python tools/probes/ab_bitwise.py gpurun_out/b.npy --compare gpurun_out/a.npy

With ``--metrics composite,spectral,bsssdr,bsseval``: every score tensor of those metrics (and
SpectralMeasures' frame values) into one .npz, the package imported from ``--root`` (a built tree;
default: this one), which locates its own libraries.  Small shapes on each side of the kernels'
chunk, group, window and piece sizes, and with ``--large`` the shapes the rate probes time.
``align``: the time alignment's outputs in its three modes, the bad intervals' realignment and the
aligned PESQ scores (align_inputs).

    python tools/probes/ab_bitwise.py a.npz --metrics composite,spectral --root other/tree
    python tools/probes/ab_bitwise.py b.npz --metrics composite,spectral --compare a.npz
"""
import argparse
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--compare")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--metrics", default="", help="comma-separated: composite, spectral, bsssdr, bsseval, align")
ap.add_argument("--root", default=os.path.join(os.path.dirname(__file__), "..", ".."),
                help="the tree to import the package (and the tests' seeded cases) from")
ap.add_argument("--large", action="store_true", help="the rate probes' shapes instead of the small ones")
a = ap.parse_args()

sys.path.insert(0, os.path.abspath(a.root))
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402


def bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def host(t):
    return t.detach().cpu().numpy()


def frame_pairs(sr: int):
    """(name, clean, denoised, lengths) for Composite and SpectralMeasures at ``sr``: one ragged batch
    of 6 rows on each side of a Composite chunk (16 hop), a Spectral group (32 hop) and one window
    (one row has no frame); and rows of more than 400 frames (the select's later passes)."""
    hop = sr * 30 // 4000
    if a.large:
        c, n, _ = speech_like_pairs(4096, 160000, sr, device="cuda", snr_low=-5, snr_high=40)
        return [("4096x160000", c, n, None)]
    cap = 2 * 32 * hop + 4 * hop
    lens = [16 * hop - 1, 16 * hop + 1, 32 * hop - 1, 32 * hop + 1, 4 * hop - 1, 4 * hop + 1]
    c, n, _ = speech_like_pairs(6, cap, sr, device="cuda", snr_low=-5, snr_high=40)
    c2, n2, _ = speech_like_pairs(2, 4 * hop + 404 * hop + 7, sr, seed=43, device="cuda", snr_low=-5, snr_high=40)
    return [("ragged", c, n, torch.tensor(lens, dtype=torch.int32)), ("long", c2, n2, None)]


def run_composite(out):
    from fast_speech_enhancement_metrics_amd import Composite
    for sr in (16000,) if a.large else (16000, 8000):
        m = Composite(sr, use_gpu=True)
        for name, c, n, lens in frame_pairs(sr):
            for key, t in zip(m.KEYS, m.scores(c, n, lengths=lens)):
                out[f"composite/{sr}/{name}/{key}"] = host(t)


def run_spectral(out):
    from fast_speech_enhancement_metrics_amd import SpectralMeasures
    for sr in (16000,) if a.large else (16000, 8000):
        m = SpectralMeasures(sr, use_gpu=True)
        for name, c, n, lens in frame_pairs(sr):
            res = m.scores(c, n, lengths=lens, return_frames=not a.large)
            for key, t in zip(m.KEYS + ("frames",), res):
                out[f"spectral/{sr}/{name}/{key}"] = host(t)


def run_bsssdr(out):
    from fast_speech_enhancement_metrics_amd import BSSSDR
    m = BSSSDR(16000, use_gpu=True)
    shapes = [(4096, 160000)] if a.large else [(3, 2047), (3, 2049), (3, 32767), (3, 32769), (3, 300)]
    for B, L in shapes:
        c, n, _ = speech_like_pairs(B, L, 16000, seed=11, device="cuda", snr_high=40.0)
        out[f"bsssdr/{B}x{L}/SDR"] = host(m.scores(c, n))


def run_bsseval(out):
    from fast_speech_enhancement_metrics_amd import BSSEval
    m = BSSEval(16000, use_gpu=True)
    names = ("SDR", "SIR", "SAR", "perm", "SDR_mat", "SIR_mat")
    if a.large:  # the shape and inputs of tools/probes/bsseval_rate.py
        B, S, L = 4096, 2, 160000
        s = speech_like_pairs(B * S, L, 16000, device="cuda", seed=3)[0].reshape(B, S, L)
        g = torch.Generator(device="cuda").manual_seed(5)
        h = torch.randn(B, S, L, generator=g, device="cuda")
        h *= 0.05 * s.abs().amax(2, keepdim=True)
        h += s
        h += 0.3 * s.sum(1, keepdim=True)
        for key, t in zip(names, m.scores(s, h, return_matrix=True)):
            out[f"bsseval/{B}x{S}x{S}x{L}/{key}"] = host(t)
        return
    from tests.bsseval_cases import mixture
    for S, E in ((1, 1), (2, 2), (3, 2)):  # (S + E odd: the group of one window signal)
        for L in (2047, 2049, 32769):
            s, h = mixture(S, E, L)
            for key, t in zip(names, m.scores(s[None].cuda(), h[None].cuda(), return_matrix=True)):
                out[f"bsseval/{S}x{E}x{L}/{key}"] = host(t)


def align_inputs():
    """(name, clean, degraded, lengths) for the time alignment: the tests' designed cases (utterances
    with known delays, three delays inside one utterance, bad intervals), a ragged batch on each
    side of the envelope frame (64), the fine stage's block (1280) and piece (5120), and rows on
    each side of the crude stages' LDS capacities (6144 envelope frames per row, 4096 per
    utterance window)."""
    from tests import align_cases as AC

    def delayed(x, D):  # y[n] = x[n - D] inside the row, else 0
        y = np.roll(x, D)
        if D > 0:
            y[:D] = 0
        elif D < 0:
            y[D:] = 0
        return y

    def pairs(B, L, seed, D):
        c, n, _ = speech_like_pairs(B, L, 16000, seed=seed)
        return c.numpy(), np.stack([delayed(n[b].numpy(), int(D[b])) for b in range(B)])

    yield ("cases",) + AC.batch() + (None,)
    yield ("cases11",) + AC.batch(seed0=11) + ([AC.L_UTT, 50000, 0, 700],)
    rows = [AC.continuous_pair(3 + k, AC.L_CONT, AC.CONT_PIECES) for k in range(4)]
    yield "continuous", np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), None
    yield ("bad",) + AC.bad_batch() + (None,)
    yield ("ragged",) + pairs(8, 40001, 32, [0, 5, -7, 300, -200, 1000, -1500, 2500]) + (
        [0, 63, 64, 1279, 1281, 5119, 5121, 40001],)
    L = 64 * 6146
    yield ("long_rows",) + pairs(2, L, 37, [2345, -610]) + ([L, L - 128],)
    L = 64 * 4200
    rows = [AC.continuous_pair(21 + b, L, [(0, L, D)]) for b, D in enumerate([700, -450])]
    yield "long_utterances", np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), [L, 64 * 4000]


def run_align(out):
    from fast_speech_enhancement_metrics_amd import PESQ
    from fast_speech_enhancement_metrics_amd.alignment import realign_bad_intervals, time_align, time_align_segments
    for name, c, d, lens in align_inputs():
        ct, dt = torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda()
        lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
        for key, t in zip(("aligned", "delay"), time_align(ct, dt, lengths=lens)):
            out[f"align/{name}/row/{key}"] = host(t)
        for mode in ("utterance", "p862"):
            seg = time_align_segments(ct, dt, lengths=lens, mode=mode)
            for key, t in zip(("aligned", "delay", "n_seg", "seg_start", "seg_delay"), seg):
                out[f"align/{name}/{mode}/{key}"] = host(t)
        m = PESQ(16000, use_gpu=True, time_align="p862")
        fr1 = m.frame_disturbances(ct, seg[0], lengths=lens)[2]
        bad = realign_bad_intervals(ct, dt, seg[0], fr1, *seg[2:], lengths=lens)
        for key, t in zip(("n_bad", "bad", "second"), bad):
            out[f"align/{name}/bad/{key}"] = host(t)
        for mode in ("row", "utterance", "p862"):
            s = PESQ(16000, use_gpu=True, time_align=mode).scores(ct, dt, lengths=lens)
            out[f"align/{name}/pesq/{mode}"] = host(s)


if not a.metrics:
    from fast_speech_enhancement_metrics_amd import PESQ_STOI
    c, n, _ = speech_like_pairs(a.batch, 160000, device="cuda")
    m = PESQ_STOI(16000, use_gpu=True)
    s = np.stack([t.cpu().numpy() for t in m.scores(c, n)])
    np.save(a.out, s)
    if a.compare:
        r = np.load(a.compare)
        same = np.array_equal(s.view(np.uint32), r.view(np.uint32))
        print("bitwise equal" if same else f"DIFFER: max |d| {np.nanmax(np.abs(s - r), axis=1)}")
        sys.exit(0 if same else 1)
    sys.exit(0)

res = {}
for name in a.metrics.split(","):
    {"composite": run_composite, "spectral": run_spectral, "bsssdr": run_bsssdr, "bsseval": run_bsseval,
     "align": run_align}[name](res)
torch.cuda.synchronize()
np.savez(a.out, **res)
if a.compare:
    ref = np.load(a.compare)
    bad = sorted(set(ref.files) ^ set(res))
    for key in sorted(set(ref.files) & set(res)):
        same = ref[key].shape == res[key].shape and np.array_equal(bits(res[key]), bits(ref[key]))
        nan = int(np.isnan(res[key]).sum()) if res[key].dtype.kind == "f" else 0
        print(f"{key} {list(res[key].shape)} ({nan} NaN): " + ("bitwise equal" if same else "DIFFER"))
        if not same:
            bad.append(key)
    for key in bad:
        print("DIFFER or missing:", key)
    sys.exit(1 if bad else 0)
