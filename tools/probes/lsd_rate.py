"""Rate of LSD.scores (csrc/lsd.hip) beside the package's own torch formulation of the same number
on the same device tensors: ``_cpu.lsd``'s operations (float64 inside, ``torch.stft``), and the
same operations in float32 (what the reference computes).  HIP events, 3 warm-up calls of the
engine and one of each formulation, the median of ``--reps`` engine calls and ``--torch-reps``
calls of each formulation.  Shape: the bench's headline shape (4096 x 160000 at 16 kHz).

    python tools/probes/lsd_rate.py [--reps 20] [--out profiles/lsd_a/lsd_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import LSD, _cpu  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

SPEC_BW = 8.0e12   # HBM3E spec, bytes/s (the bench roofline's convention)


def torch_float32(s: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """_cpu.lsd's operations without the float64 copies."""
    a = (s * h).sum(1, keepdim=True) / (h.square().sum(1, keepdim=True) + 1e-8)
    x = torch.cat([s, h * a])
    w = torch.hann_window(512, dtype=torch.float32, device=x.device)
    mag = torch.stft(x, n_fft=512, hop_length=256, window=w, center=True, pad_mode="constant",
                     return_complex=True).abs()
    S, H = mag[:s.shape[0]], mag[s.shape[0]:]
    return torch.log(S.square() / (H + 1e-8).square() + 1e-8).square().mean(1).sqrt().mean(1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "lsd_a", "lsd_rate.json"))
    ap.add_argument("--shapes", default="4096x160000")
    a = ap.parse_args()
    sr = 16000
    m = LSD(sr, use_gpu=True)
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        torch.cuda.synchronize()
        for _ in range(3):
            eng = m.scores(c, n)
        ref64 = _cpu.lsd(c, n)
        ref32 = torch_float32(c, n)
        torch.cuda.synchronize()
        te = [timed(lambda: m.scores(c, n))[0] for _ in range(a.reps)]
        t64 = [timed(lambda: _cpu.lsd(c, n))[0] for _ in range(a.torch_reps)]
        t32 = [timed(lambda: torch_float32(c, n))[0] for _ in range(a.torch_reps)]
        ms_e, ms_64, ms_32 = statistics.median(te), statistics.median(t64), statistics.median(t32)
        rel = lambda x: float(((x.double() - ref64.double()).abs() / ref64.double()).max())  # noqa: E731
        nbytes = 2 * B * L * 4
        out["shapes"][shape] = {
            "engine": {"ms_per_call": round(ms_e, 4), "utterances_per_s": round(B / ms_e * 1e3, 1),
                       "algorithmic_bytes": nbytes, "TB_per_s": round(nbytes / ms_e / 1e9, 3),
                       "share_of_8TBps_spec": round(nbytes / (ms_e * 1e-3) / SPEC_BW, 4)},
            "torch_formulation_float64": {"ms_per_call": round(ms_64, 4),
                                          "utterances_per_s": round(B / ms_64 * 1e3, 1)},
            "torch_formulation_float32": {"ms_per_call": round(ms_32, 4),
                                          "utterances_per_s": round(B / ms_32 * 1e3, 1)},
            "engine_speedup_vs_float64": round(ms_64 / ms_e, 2),
            "engine_speedup_vs_float32": round(ms_32 / ms_e, 2),
            "worst_rel_engine_vs_float64": rel(eng),
            "worst_rel_float32_vs_float64": rel(ref32),
        }
        del c, n, eng, ref64, ref32
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
