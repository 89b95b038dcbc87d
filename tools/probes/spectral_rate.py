"""Rate of SpectralMeasures.scores (fwSegSNR, CD, IS; csrc/spectral.hip) beside Composite.scores and
PESQ.scores on the same device tensors in the same process, and beside the same definitions written
with torch ops on the device tensors (``_cpu.spectral`` on CUDA rows, float64, ``--torch-rows`` rows
of the batch).  Composite's frame kernels (composite_frames and composite_rows: LLR, WSS, SegSNR on
the same frames, window and LPC orders) cost Composite.scores minus PESQ.scores; that difference
per frame is the figure the new frame kernel is reported against.  HIP events, 3 warm-up calls, the
median of ``--reps`` calls of each, alternating.  Shapes: the bench's headline shape (4096 x 160000
at 16 kHz) and 64 x 256000.  The per-kernel split comes from a kernel trace taken in a run of its
own (rocprofv3 --kernel-trace --stats -- python tools/probes/spectral_rate.py --reps 3
--torch-rows 0 --out "").

    python tools/probes/spectral_rate.py [--reps 20] [--out profiles/spectral_a/spectral_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import PESQ, Composite, SpectralMeasures, _cpu  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join("profiles", "spectral_a", "spectral_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    ap.add_argument("--torch-rows", type=int, default=16)
    a = ap.parse_args()
    sr = 16000
    s, m, p = SpectralMeasures(sr, use_gpu=True), Composite(sr, use_gpu=True), PESQ(sr, use_gpu=True)
    out = {"sample_rate": sr, "reps": a.reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        torch.cuda.synchronize()
        for _ in range(3):
            spec = s.scores(c, n)
            m.scores(c, n)
            p.scores(c, n)
        torch.cuda.synchronize()
        ts, tc, tp = [], [], []
        for _ in range(a.reps):
            ts.append(timed(lambda: s.scores(c, n))[0])
            tc.append(timed(lambda: m.scores(c, n))[0])
            tp.append(timed(lambda: p.scores(c, n))[0])
        ms_s, ms_c, ms_p = statistics.median(ts), statistics.median(tc), statistics.median(tp)
        frames = B * s.frames_of(L)
        rec = {
            "frames": frames,
            "spectral": {"ms_per_call": round(ms_s, 4), "ns_per_frame": round(ms_s * 1e6 / frames, 2),
                         "utterances_per_s": round(B / ms_s * 1e3, 1)},
            "composite": {"ms_per_call": round(ms_c, 4), "ns_per_frame": round(ms_c * 1e6 / frames, 2)},
            "pesq_alone": {"ms_per_call": round(ms_p, 4)},
            "composite_minus_pesq": {"ms_per_call": round(ms_c - ms_p, 4),
                                     "ns_per_frame": round((ms_c - ms_p) * 1e6 / frames, 2)},
            "nonfinite_scores": int(sum((~torch.isfinite(v)).sum() for v in spec)),
        }
        if a.torch_rows:
            R = min(a.torch_rows, B)
            ct, nt = c[:R], n[:R]
            ref = _cpu.spectral(ct, nt, sr)
            torch.cuda.synchronize()
            tt = [timed(lambda: _cpu.spectral(ct, nt, sr))[0] for _ in range(3)]
            ms_t = statistics.median(tt)
            rec["torch_ops"] = {"rows": R, "ms_per_call": round(ms_t, 3),
                                "ns_per_frame": round(ms_t * 1e6 / (R * s.frames_of(L)), 1),
                                "worst_abs_diff_to_engine": [round(float((ref[k].float() - spec[k][:R]).abs().max()), 7)
                                                             for k in range(3)]}
        out["shapes"][shape] = rec
        del c, n, spec
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
