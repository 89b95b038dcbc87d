"""Rate of DNSMOS.scores (csrc/dnsmos.hip) beside the package's own torch formulation of the same
network on the same device tensors: float32 front end, the convolution stack and the dense layers
under float16 autocast (MIOpen / hipBLASLt), once batched over segments (``--chunk`` segments per
forward) and once looped per utterance, as the reference does.  HIP events; one warm-up call of
each, the median of ``--reps`` engine calls and ``--torch-reps`` calls of each formulation.  The
per-utterance loop runs on the first ``--loop-rows`` rows and is scaled to the batch (stated in
the output).  Shapes: 4096 x 10 s (one segment per row) and 64 x 16 s (seven segments per row).

    python tools/probes/dnsmos_rate.py [--reps 5] [--out profiles/dnsmos_a/dnsmos_rate.json]

The per-kernel split comes from a kernel trace of a short engine-only run
(``--engine-only --shapes 256x160000 --reps 2`` under ``rocprofv3 --kernel-trace --stats``).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import DNSMOS, _cpu  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

GFLOP_PER_SEGMENT = 38.8   # the seven convolutions of one 900 x 161 image
DENSE_F16_PEAK = 2.5e15    # MI355X dense f16 / bf16 MFMA, FLOP/s


def torch_scores(w: dict, rows: torch.Tensor, chunk: int) -> torch.Tensor:
    """[B, 3] scores of equal-length rows of at least 144160 samples, `chunk` segments per forward."""
    B = rows.shape[0]
    segs = rows.unfold(1, _cpu.DNSMOS_SEGMENT, _cpu.DNSMOS_HOP)
    per_row = segs.shape[1]
    segs = segs.reshape(-1, _cpu.DNSMOS_SEGMENT)
    raws = []
    with torch.no_grad():
        for i in range(0, segs.shape[0], chunk):
            img = _cpu.dnsmos_features(w, segs[i:i + chunk])
            with torch.autocast("cuda", dtype=torch.float16):
                raws.append(_cpu.dnsmos_network(w, img).float())
    raw = torch.cat(raws)
    c0, c1, c2 = (torch.tensor(c, dtype=torch.float32, device=raw.device) for c in _cpu._DNSMOS_POLY)
    return (c0 + c1 * raw + c2 * raw.square()).reshape(B, per_row, 3).mean(1)


def torch_per_utterance(w: dict, rows: torch.Tensor) -> torch.Tensor:
    return torch.cat([torch_scores(w, rows[b:b + 1], 1 << 30) for b in range(rows.shape[0])])


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
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--loop-rows", type=int, default=128)
    ap.add_argument("--check-rows", type=int, default=128)
    ap.add_argument("--engine-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "dnsmos_a", "dnsmos_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    a = ap.parse_args()
    sr = 16000
    m = DNSMOS(sr, use_gpu=True)
    w = {k: v.cuda() for k, v in m.weights.items()}
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps, "torch_chunk_segments": a.chunk,
           "gflop_per_segment": GFLOP_PER_SEGMENT, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        _, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        nseg = B * _cpu.dnsmos_segments(L)
        flop = nseg * GFLOP_PER_SEGMENT * 1e9
        torch.cuda.synchronize()
        eng = m.scores(n)
        torch.cuda.synchronize()
        ms_e = statistics.median([timed(lambda: m.scores(n))[0] for _ in range(a.reps)])
        rec = {"segments": nseg,
               "engine": {"ms_per_call": round(ms_e, 3), "utterances_per_s": round(B / ms_e * 1e3, 1),
                          "f16_TFLOP_per_s": round(flop / ms_e / 1e9, 1),
                          "share_of_2.5PF_dense": round(flop / (ms_e * 1e-3) / DENSE_F16_PEAK, 4)}}
        if not a.engine_only:
            k = min(B, a.loop_rows)
            ref = torch_scores(w, n, a.chunk)
            torch_per_utterance(w, n[:2])
            torch.cuda.synchronize()
            ms_b = statistics.median([timed(lambda: torch_scores(w, n, a.chunk))[0] for _ in range(a.torch_reps)])
            ms_l = statistics.median([timed(lambda: torch_per_utterance(w, n[:k]))[0] for _ in range(a.torch_reps)])
            ms_l *= B / k
            rec["torch_f16_autocast_batched"] = {"ms_per_call": round(ms_b, 3),
                                                 "utterances_per_s": round(B / ms_b * 1e3, 1),
                                                 "f16_TFLOP_per_s": round(flop / ms_b / 1e9, 1)}
            rec["torch_f16_autocast_per_utterance"] = {"ms_per_call": round(ms_l, 3), "rows_timed": k,
                                                       "scaled_to_rows": B,
                                                       "utterances_per_s": round(B / ms_l * 1e3, 1),
                                                       "f16_TFLOP_per_s": round(flop / ms_l / 1e9, 1)}
            rec["engine_speedup_vs_torch_batched"] = round(ms_b / ms_e, 3)
            rec["engine_speedup_vs_torch_per_utterance"] = round(ms_l / ms_e, 3)
            rec["worst_abs_engine_vs_torch_batched"] = float((eng - ref).abs().max())
            # which of the two is off: both against the same formulation in float32 on the first rows
            kc = min(B, a.check_rows)
            with torch.no_grad():
                segs = n[:kc].unfold(1, _cpu.DNSMOS_SEGMENT, _cpu.DNSMOS_HOP)
                raw32 = torch.cat([_cpu.dnsmos_network(w, _cpu.dnsmos_features(w, segs[b])) for b in range(kc)])
            c0, c1, c2 = (torch.tensor(c, dtype=torch.float32, device="cuda") for c in _cpu._DNSMOS_POLY)
            ref32 = (c0 + c1 * raw32 + c2 * raw32.square()).reshape(kc, -1, 3).mean(1)
            rec["float32_check"] = {"rows": kc, "worst_abs_engine": float((eng[:kc] - ref32).abs().max()),
                                    "worst_abs_torch_f16_batched": float((ref[:kc] - ref32).abs().max())}
            del ref, ref32, raw32
        out["shapes"][shape] = rec
        del n, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
