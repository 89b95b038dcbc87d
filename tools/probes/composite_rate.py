"""Rate of Composite.scores (CSIG, CBAK, COVL with PESQ, LLR, WSS, SegSNR; csrc/composite.hip)
beside PESQ.scores alone on the same device tensors in the same process: the composite's added
cost is the measured difference against the existing PESQ path.  HIP events, 3 warm-up calls, the
median of ``--reps`` calls of each, alternating.  Shapes: the bench's headline shape (4096 x 160000
at 16 kHz) and the reference's own benchmark setting (64 x 256000); the CPU mode is timed at batch
64 (``--cpu-rows``, one call, host clock).  The per-kernel split comes from a kernel trace taken in
a run of its own (rocprofv3 --kernel-trace --stats -- python tools/probes/composite_rate.py
--reps 3 --cpu-rows 0 --out "").

    python tools/probes/composite_rate.py [--reps 20] [--out profiles/composite_a/composite_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import PESQ, Composite  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join("profiles", "composite_a", "composite_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    ap.add_argument("--cpu-rows", type=int, default=64)
    a = ap.parse_args()
    sr = 16000
    m, p = Composite(sr, use_gpu=True), PESQ(sr, use_gpu=True)
    out = {"sample_rate": sr, "reps": a.reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        torch.cuda.synchronize()
        for _ in range(3):
            comp = m.scores(c, n)
            mos = p.scores(c, n)
        torch.cuda.synchronize()
        tc, tp = [], []
        for _ in range(a.reps):
            tc.append(timed(lambda: m.scores(c, n))[0])
            tp.append(timed(lambda: p.scores(c, n))[0])
        ms_c, ms_p = statistics.median(tc), statistics.median(tp)
        hop = sr * 30 // 4000
        frames = B * ((L - 4 * hop) // hop + 1)
        out["shapes"][shape] = {
            "composite": {"ms_per_call": round(ms_c, 4), "utterances_per_s": round(B / ms_c * 1e3, 1)},
            "pesq_alone": {"ms_per_call": round(ms_p, 4), "utterances_per_s": round(B / ms_p * 1e3, 1)},
            "added_ms_per_call": round(ms_c - ms_p, 4),
            "added_over_pesq": round((ms_c - ms_p) / ms_p, 3),
            "frames": frames,
            "added_ns_per_frame": round((ms_c - ms_p) * 1e6 / frames, 2),
            "pesq_key_equals_pesq_class": bool(torch.equal(comp[3], mos)),
            "nonfinite_scores": int(sum((~torch.isfinite(v)).sum() for v in comp)),
        }
        if a.cpu_rows and B >= a.cpu_rows and "cpu_mode" not in out:
            ch, nh = c[:a.cpu_rows].cpu(), n[:a.cpu_rows].cpu()
            cpu = Composite(sr, use_gpu=False)
            t0 = time.perf_counter()
            cpu.scores(ch, nh)
            out["cpu_mode"] = {"rows": a.cpu_rows, "length": L, "ms_per_call": round((time.perf_counter() - t0) * 1e3, 1)}
        del c, n, comp, mos
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
