"""Rate of SDR.scores (SI-SDR, SNR, segmental SNR; csrc/sdr.hip) beside a torch-ops formulation of
the same three numbers on the same device tensors -- what a user of the package writes without
the engine: float32 sums, ``unfold`` for the frames.  HIP events, 3 warm-up calls, the median of
``--reps`` calls of each, alternating.  Shapes: the bench's headline shape (4096 x 160000 at
16 kHz) and the reference's own benchmark setting (64 x 256000).

    python tools/probes/sdr_rate.py [--reps 20] [--out profiles/sdr_a/sdr_rate.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import SDR  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

SPEC_BW = 8.0e12   # HBM3E spec, bytes/s (the bench roofline's convention)
COPY_BW = 6.29e12  # measured float4 copy on the MI355X


def torch_formulation(s: torch.Tensor, h: torch.Tensor, sr: int):
    """(si_sdr, snr, seg_snr) [B] float32 with torch ops, float32 sums."""
    d = h - s
    ss, sn, nn = (s * s).sum(1), (s * h).sum(1), (h * h).sum(1)
    snr = 10 * torch.log10(ss / (d * d).sum(1))
    t = sn * sn / ss
    si = 10 * torch.log10(t / (nn - t).clamp_min(0))
    hop = sr * 30 // 4000
    win = 4 * hop
    w = 0.5 * (1 - torch.cos(2 * math.pi * torch.arange(1, win + 1, device=s.device, dtype=torch.float32) / (win + 1)))
    es = (s.unfold(1, win, hop) * w).square().sum(2)
    ed = (d.unfold(1, win, hop) * w).square().sum(2)
    seg = (10 * torch.log10(es / (ed + 1e-10) + 1e-10)).clamp(-10, 35).mean(1)
    return si, snr, seg


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
    ap.add_argument("--out", default=os.path.join("profiles", "sdr_a", "sdr_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    a = ap.parse_args()
    sr = 16000
    m = SDR(sr, use_gpu=True)
    out = {"sample_rate": sr, "reps": a.reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        torch.cuda.synchronize()
        for _ in range(3):
            eng = m.scores(c, n)
            ref = torch_formulation(c, n, sr)
        torch.cuda.synchronize()
        te, tt = [], []
        for _ in range(max(a.reps, 20)):
            te.append(timed(lambda: m.scores(c, n))[0])
            tt.append(timed(lambda: torch_formulation(c, n, sr))[0])
        ms_e, ms_t = statistics.median(te), statistics.median(tt)
        worst = {}
        for key, e, r in zip(SDR.KEYS, eng, ref):
            both = torch.isfinite(e) & torch.isfinite(r)
            worst[key] = float((e[both].double() - r[both].double()).abs().max()) if bool(both.any()) else None
            worst[key + "_torch_nonfinite_rows"] = int((~torch.isfinite(r)).sum())
        nbytes = 2 * B * L * 4
        out["shapes"][shape] = {
            "engine": {"ms_per_call": round(ms_e, 4), "utterances_per_s": round(B / ms_e * 1e3, 1),
                       "algorithmic_bytes": nbytes, "TB_per_s": round(nbytes / ms_e / 1e9, 3),
                       "share_of_8TBps_spec": round(nbytes / (ms_e * 1e-3) / SPEC_BW, 4),
                       "share_of_6.29TBps_copy": round(nbytes / (ms_e * 1e-3) / COPY_BW, 4)},
            "torch_formulation": {"ms_per_call": round(ms_t, 4), "utterances_per_s": round(B / ms_t * 1e3, 1)},
            "engine_speedup": round(ms_t / ms_e, 2),
            "worst_abs_engine_minus_torch_dB": worst,
        }
        del c, n, eng, ref
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
