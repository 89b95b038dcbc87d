"""Rate of BSSSDR.scores (csrc/bsssdr.hip) beside the same definition written with torch operations on
the same device tensors: the float32 normalisation, ``torch.fft`` correlations in float64 with the
reference's transform length, the explicit 512 x 512 Toeplitz matrices and a float64 Cholesky
factorisation (``torch.linalg.cholesky_ex`` + ``torch.cholesky_solve``; no ``linalg.solve``), in
slabs of ``--slab`` rows so that the spectra and the matrices fit beside the inputs.  HIP events,
3 warm-up calls of the engine and one of the formulation, the median of ``--reps`` engine calls and
``--torch-reps`` calls of the formulation.  Shapes: the bench's headline shape (4096 x 160000 at
16 kHz) and 64 x 256000 (16 s rows).

    python tools/probes/bsssdr_rate.py [--reps 10] [--out profiles/bsssdr_a/bsssdr_rate.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import BSSSDR  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

K = 512
PEAK_FP64 = 78.6e12  # MI355X vector FP64 peak, FLOP/s (public specification)


def torch_formulation(s: torch.Tensor, h: torch.Tensor, slab: int):
    """([B] float64 SDR, rows whose factorisation failed) of the definition with torch operations."""
    out, failed = [], 0
    idx = (torch.arange(K, device=s.device)[None] - torch.arange(K, device=s.device)[:, None]).abs()
    n_fft = 2 ** math.ceil(math.log2(2 * s.shape[1] - 1))
    for b0 in range(0, s.shape[0], slab):
        sb, hb = s[b0:b0 + slab], h[b0:b0 + slab]
        ns = sb.double().square().sum(1).sqrt().float().clamp(min=1e-6)
        nh = hb.double().square().sum(1).sqrt().float().clamp(min=1e-6)
        sd, hd = (sb / ns[:, None]).double(), (hb / nh[:, None]).double()
        Sf = torch.fft.rfft(sd, n=n_fft)
        r = torch.fft.irfft(Sf.abs().square(), n=n_fft)[:, :K]
        b = torch.fft.irfft(Sf.conj() * torch.fft.rfft(hd, n=n_fft), n=n_fft)[:, :K]
        del Sf
        fac, info = torch.linalg.cholesky_ex(r[:, idx])
        x = torch.cholesky_solve(b[:, :, None], fac)[:, :, 0]
        coh = (b * x).sum(1)
        val = 10.0 * torch.log10((coh / (1.0 - coh).clamp(min=1e-8)).clamp(min=1e-8))
        out.append(torch.where(info == 0, val, torch.full_like(val, float("nan"))))
        failed += int((info != 0).sum())
    return torch.cat(out), failed


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--slab", type=int, default=128)
    ap.add_argument("--out", default=os.path.join("profiles", "bsssdr_a", "bsssdr_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    ap.add_argument("--no-torch", action="store_true", help="time the engine only")
    a = ap.parse_args()
    sr = 16000
    m = BSSSDR(sr, use_gpu=True)
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps, "slab": a.slab, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        torch.cuda.synchronize()
        for _ in range(3):
            eng = m.scores(c, n)
        torch.cuda.synchronize()
        te = [timed(lambda: m.scores(c, n))[0] for _ in range(a.reps)]
        ms_e = statistics.median(te)
        flop = 2 * 2 * K * B * L  # the two correlations' multiply-adds
        rec = {"engine": {"ms_per_call": round(ms_e, 4), "min_ms": round(min(te), 4), "max_ms": round(max(te), 4),
                          "utterances_per_s": round(B / ms_e * 1e3, 1), "correlation_flop": flop,
                          "TFLOP_per_s_fp64": round(flop / ms_e / 1e9, 2),
                          "share_of_fp64_vector_peak": round(flop / (ms_e * 1e-3) / PEAK_FP64, 4),
                          "nan_rows": int(torch.isnan(eng).sum())}}
        print(shape, json.dumps(rec), flush=True)
        if not a.no_torch:
            ref, failed = torch_formulation(c, n, a.slab)
            torch.cuda.synchronize()
            tt = [timed(lambda: torch_formulation(c, n, a.slab))[0] for _ in range(a.torch_reps)]
            ms_t = statistics.median(tt)
            ok = ~torch.isnan(ref) & ~torch.isnan(eng) & (ref.abs() <= 60)
            rec["torch_formulation_float64"] = {"ms_per_call": round(ms_t, 4),
                                                "utterances_per_s": round(B / ms_t * 1e3, 1),
                                                "rows_whose_cholesky_failed": failed}
            rec["engine_speedup_vs_torch_formulation"] = round(ms_t / ms_e, 2)
            rec["worst_abs_dB_engine_vs_torch_formulation"] = float((eng.double() - ref)[ok].abs().max()) if ok.any() else None
            rec["rows_compared"] = int(ok.sum())
            del ref
        out["shapes"][shape] = rec
        del c, n, eng
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
