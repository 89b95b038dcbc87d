"""Rate of SRMR.scores (csrc/srmr.hip): ms per call on device tensors for the bench's headline shape
(4096 x 160000 at 16 kHz) and 64 x 256000, the package's CPU mode (``_cpu.srmr``, float64 scipy
filters on the host's threads) on ``--cpu-rows`` rows of the second shape, and the arithmetic rates the
engine reaches.  HIP events, 2 warm-up calls, the median of ``--reps`` calls.

Operation counts per channel-sample (23 channels x the samples the frames cover), as the kernel issues
them, scans and table reads left out:
  float32: numerator 10 (2 mul + 4 fma), four stages x two passes x one complex multiply-add (4 fma)
           = 64, envelope 4  ->  78 flop;
  float64: eight filters x (first pass sub + mul + 2 fma = 6, second pass the same + mul + fma = 9)
           ->  120 flop.
Peaks: 157.3 TFLOP/s float32 vector (the MI355X guide's chip table) and 78.6 TFLOP/s float64 vector
(the public datasheet figure; half the float32 rate).

    python tools/probes/srmr_rate.py [--reps 5] [--out profiles/srmr_a/srmr_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import SRMR, _cpu  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

FLOP32, FLOP64 = 78, 120
PEAK32, PEAK64 = 157.3e12, 78.6e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "srmr_a", "srmr_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    ap.add_argument("--cpu-rows", type=int, default=64)
    a = ap.parse_args()
    sr = 16000
    m = SRMR(sr, use_gpu=True)
    out = {"sample_rate": sr, "reps": a.reps, "flop_per_channel_sample": {"float32": FLOP32, "float64": FLOP64},
           "peaks_tflops": {"float32": PEAK32 / 1e12, "float64": PEAK64 / 1e12}, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        _, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        torch.cuda.synchronize()
        for _ in range(2):
            got = m.scores(n)
        torch.cuda.synchronize()
        ms = statistics.median(timed(lambda: m.scores(n))[0] for _ in range(a.reps))
        F = m.frames_of(L)
        covered = (F - 1) * m.hop_length + m.win_length
        cs = B * m.CHANNELS * covered
        rec = {"ms_per_call": round(ms, 3), "utterances_per_s": round(B / ms * 1e3, 1),
               "audio_seconds_per_s": round(B * L / sr / ms * 1e3, 1), "channel_samples": cs,
               "ns_per_channel_sample": round(ms * 1e6 / cs, 5),
               "float32_tflops": round(cs * FLOP32 / ms / 1e9, 3), "float64_tflops": round(cs * FLOP64 / ms / 1e9, 3),
               "float32_of_peak": round(cs * FLOP32 / (ms * 1e-3) / PEAK32, 4),
               "float64_of_peak": round(cs * FLOP64 / (ms * 1e-3) / PEAK64, 4),
               "nonfinite_scores": int((~torch.isfinite(got)).sum())}
        if a.cpu_rows and B <= a.cpu_rows:
            host = n[:a.cpu_rows].cpu()
            cpu = SRMR(sr)
            t0 = time.perf_counter()
            ref = cpu.scores(host)
            t = time.perf_counter() - t0
            rel = ((ref - got[:len(host)].cpu()).abs() / ref.abs())
            rec["cpu_mode"] = {"rows": len(host), "threads": _cpu.host_threads(), "ms_per_call": round(t * 1e3, 1),
                               "worst_relative_diff_to_engine": float(rel[torch.isfinite(rel)].max())}
        out["shapes"][shape] = rec
        del n, got
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
