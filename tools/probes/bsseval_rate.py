"""Rate of BSSEval.scores (csrc/bsseval.hip) at S = E = 2 beside the same definition written with torch
operations on the same device tensors -- the float32 normalisation, ``torch.fft`` correlations in
float64, the explicit S 512 x S 512 Gram matrices and float64 Cholesky factorisations
(``torch.linalg.cholesky_ex`` + ``solve_triangular``), in slabs of ``--slab`` mixtures -- and, at
S = E = 1, beside BSSSDR.scores on the same rows in the same process.  HIP events, 3 warm-up calls
of the engine and one of the formulation, the median of ``--reps`` engine calls and ``--torch-reps``
calls of the formulation.  Shapes: 4096 mixtures of 10 s and 64 of 16 s at 16 kHz.

The correlation kernel's own time is not measured apart: it is taken as the call's time less the
time of a call on the same number of mixtures of 1024 samples (one LDS piece each: the recursions
and the fixed stages, which do not depend on the length), and said to be derived.

    python tools/probes/bsseval_rate.py [--reps 10] [--out profiles/bsseval_a/bsseval_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import BSSSDR, BSSEval  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

K = 512
PEAK_FP64 = 78.6e12  # MI355X vector FP64 peak, FLOP/s (public specification)


def mixtures(B: int, S: int, L: int, sr: int):
    """(sources [B, S, L], estimates [B, S, L]) on the device: estimate e is source e plus 0.3 of the
    sources' sum plus white noise at 0.05 of its peak."""
    s = speech_like_pairs(B * S, L, sr, device="cuda", seed=3)[0].reshape(B, S, L)
    g = torch.Generator(device="cuda").manual_seed(5)
    h = torch.randn(B, S, L, generator=g, device="cuda")
    h *= 0.05 * s.abs().amax(2, keepdim=True)
    h += s
    h += 0.3 * s.sum(1, keepdim=True)
    return s, h


def torch_formulation(s: torch.Tensor, h: torch.Tensor, slab: int):
    """(SDR, SIR [B, S, E], SAR [B, E] float64, mixtures whose factorisation failed) with torch operations."""
    B, S, L = s.shape
    E = h.shape[1]
    nfft = 1 << (L + K - 1).bit_length()
    lag = torch.arange(K, device=s.device)[:, None] - torch.arange(K, device=s.device)[None, :] + K - 1
    outs, failed = [], 0

    def db(num, den):
        return 10.0 * torch.log10((num / den.clamp(min=1e-8)).clamp(min=1e-8))

    def unit(x):
        nrm = x.double().square().sum(-1).sqrt().float().clamp(min=1e-6)
        return (x / nrm[..., None]).double()

    for b0 in range(0, B, slab):
        Sf = torch.fft.rfft(unit(s[b0:b0 + slab]), n=nfft)
        Hf = torch.fft.rfft(unit(h[b0:b0 + slab]), n=nfft)
        C = torch.fft.irfft(Sf.conj()[:, :, None] * Sf[:, None], n=nfft)[..., :K]
        b = torch.fft.irfft(Sf.conj()[:, :, None] * Hf[:, None], n=nfft)[..., :K]
        del Sf, Hf
        full = torch.cat([C.transpose(1, 2).flip(3)[..., :-1], C], 3)
        nb = C.shape[0]
        G = full[:, :, :, lag].permute(0, 1, 3, 2, 4).reshape(nb, S * K, S * K)
        d = b.permute(0, 1, 3, 2).reshape(nb, S * K, E)
        fac, info = torch.linalg.cholesky_ex(G)
        y = torch.linalg.solve_triangular(fac, d, upper=False)
        coh_all = (y * y).sum(1)
        coh = []
        for i in range(S):
            fi, inf_i = torch.linalg.cholesky_ex(G[:, i * K:(i + 1) * K, i * K:(i + 1) * K])
            yi = torch.linalg.solve_triangular(fi, d[:, i * K:(i + 1) * K], upper=False)
            coh.append((yi * yi).sum(1))
            info = info | inf_i
        coh = torch.stack(coh, 1)
        outs.append((db(coh, 1 - coh), db(coh, coh_all[:, None] - coh), db(coh_all, 1 - coh_all)))
        failed += int((info != 0).sum())
        del G, fac, y
    return tuple(torch.cat([o[k] for o in outs]) for k in range(3)) + (failed,)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def median_ms(fn, reps: int, warm: int = 3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn)[0] for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--slab", type=int, default=64)
    ap.add_argument("--out", default=os.path.join("profiles", "bsseval_a", "bsseval_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    ap.add_argument("--no-torch", action="store_true", help="time the engine only")
    a = ap.parse_args()
    sr, S = 16000, 2
    m = BSSEval(sr, use_gpu=True)
    out = {"sample_rate": sr, "sources": S, "estimates": S, "reps": a.reps, "torch_reps": a.torch_reps, "slab": a.slab,
           "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        s, h = mixtures(B, S, L, sr)
        torch.cuda.synchronize()
        ms_e, lo, hi = median_ms(lambda: m.scores(s, h, return_matrix=True), a.reps)
        eng = m.scores(s, h, return_matrix=True)
        ms_fixed, _, _ = median_ms(lambda: m.scores(s[:, :, :1024], h[:, :, :1024]), a.reps)
        flop = 2 * (S * S + S * S) * K * B * L  # the S^2 + S E correlations' multiply-adds
        ms_corr = ms_e - ms_fixed
        rec = {"engine": {"ms_per_call": round(ms_e, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                          "mixtures_per_s": round(B / ms_e * 1e3, 1), "nan_mixtures": int(torch.isnan(eng[2]).any(1).sum()),
                          "ms_per_call_at_1024_samples": round(ms_fixed, 4),
                          "correlation_flop": flop,
                          "TFLOP_per_s_fp64_whole_call": round(flop / ms_e / 1e9, 2),
                          "correlation_ms_derived": round(ms_corr, 4),
                          "correlation_TFLOP_per_s_fp64_derived": round(flop / ms_corr / 1e9, 2),
                          "correlation_share_of_fp64_vector_peak_derived": round(flop / (ms_corr * 1e-3) / PEAK_FP64, 4)}}
        print(shape, json.dumps(rec), flush=True)
        if not a.no_torch:
            ref = torch_formulation(s, h, a.slab)
            torch.cuda.synchronize()
            tt = [timed(lambda: torch_formulation(s, h, a.slab))[0] for _ in range(a.torch_reps)]
            ms_t = statistics.median(tt)
            worst = 0.0
            for g, r in ((eng[4], ref[0]), (eng[5], ref[1]), (eng[2], ref[2])):
                ok = ~torch.isnan(r) & ~torch.isnan(g) & (r.abs() <= 60)
                worst = max(worst, float((g.double() - r)[ok].abs().max()) if ok.any() else 0.0)
            rec["torch_formulation_float64"] = {"ms_per_call": round(ms_t, 4), "mixtures_per_s": round(B / ms_t * 1e3, 1),
                                                "mixtures_whose_cholesky_failed": ref[3]}
            rec["engine_speedup_vs_torch_formulation"] = round(ms_t / ms_e, 2)
            rec["worst_abs_dB_engine_vs_torch_formulation"] = worst
            del ref
        # S = E = 1 beside BSSSDR on the same rows
        c, n = s[:, 0].contiguous(), h[:, 0].contiguous()
        one = BSSSDR(sr, use_gpu=True)
        ms_b, _, _ = median_ms(lambda: one.scores(c, n), a.reps)
        ms_1, _, _ = median_ms(lambda: m.scores(c, n), a.reps)
        ms_1f, _, _ = median_ms(lambda: m.scores(c[:, :1024], n[:, :1024]), a.reps)
        ms_bf, _, _ = median_ms(lambda: one.scores(c[:, :1024], n[:, :1024]), a.reps)
        d = (m.scores(c, n)[0][:, 0].double() - one.scores(c, n).double()).abs()
        rec["one_source"] = {"bsseval_ms_per_call": round(ms_1, 4), "bsssdr_ms_per_call": round(ms_b, 4),
                             "ratio": round(ms_1 / ms_b, 3), "bsseval_ms_at_1024_samples": round(ms_1f, 4),
                             "bsssdr_ms_at_1024_samples": round(ms_bf, 4),
                             "worst_abs_dB_bsseval_vs_bsssdr": float(d[~torch.isnan(d)].max())}
        print(shape, json.dumps(rec["one_source"]), flush=True)
        out["shapes"][shape] = rec
        del s, h, c, n, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
