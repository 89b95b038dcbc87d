"""Rate of BSSSDR.loss + backward (csrc/bsssdr_grad.hip) beside BSSSDR.scores on the same rows (the forward
alone) and beside the same definition written in torch ops on the same device tensors with autograd -- float64
(the reference) and float32 (what a training script would write): the float32 normalisation, ``torch.fft``
correlations and a dense solve of the 512 x 512 Toeplitz system -- with the gradient error of the engine and of
the float32 form against float64 (max over a row of |g - g_ref| / max|g_ref|, the worst row).  HIP events, 3
warm-up calls, the median of ``--reps`` calls.  Shapes: B x L at 16 kHz, by default the bench's headline shape
4096 x 10 s and 64 x 16 s.  The torch forms run on the first ``--torch-batch`` rows and their times are scaled to
the batch.

    python tools/probes/bsssdr_loss_rate.py [--reps 10] [--out profiles/bsssdr_loss_a/bsssdr_loss_rate.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import BSSSDR, _native  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

K = 512


def torch_loss(c, est, dtype):
    """-mean SDR of 16 kHz rows [B, L] in ``dtype`` on the rows' device: the definition of
    include/fsem_bsssdr.h in torch ops (the float32 quotients as constants of the rounding: the estimate's
    quotient is taken in ``dtype``, which is the smooth normalisation the engine's backward differentiates)."""
    s = c / c.double().square().sum(1, keepdim=True).sqrt().float().clamp(min=1e-6)
    s, h = s.to(dtype), est.to(dtype)
    h = h / h.square().sum(1, keepdim=True).sqrt().clamp(min=1e-6)
    n_fft = 2 ** math.ceil(math.log2(2 * s.shape[1] - 1))
    Sf = torch.fft.rfft(s, n=n_fft)
    r = torch.fft.irfft(Sf.abs().square(), n=n_fft)[:, :K]
    b = torch.fft.irfft(Sf.conj() * torch.fft.rfft(h, n=n_fft), n=n_fft)[:, :K]
    lag = torch.arange(K, device=s.device)
    x = torch.linalg.solve(r[:, (lag[None] - lag[:, None]).abs()], b)
    coh = (b * x).sum(1)
    return -(10.0 * torch.log10((coh / (1.0 - coh).clamp(min=1e-8)).clamp(min=1e-8))).mean()


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
    return statistics.median(timed(fn)[0] for _ in range(reps))


def loss_backward(m, c, est):
    est.grad = None
    m.loss(c, est).backward()
    return est.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-batch", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "bsssdr_loss_a", "bsssdr_loss_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    a = ap.parse_args()
    sr = 16000
    m = BSSSDR(sr, use_gpu=True)
    lib, blib = _native.load(), _native.load_bsssdr()
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps,
           "note": "the torch forms normalise the estimate in their own dtype; the engine differentiates at the "
                   "float32 quotients the score is taken at, so its distance from torch_float64 includes that "
                   "difference of definition (INTEGRATION.md section 19), not rounding alone",
           "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        est = n.clone().requires_grad_(True)
        ms_f = median_ms(lambda: m.scores(c, n), a.reps)
        with torch.no_grad():
            ms_d = median_ms(lambda: m.differentiable_scores(c, n), a.reps)
        ms_fb = median_ms(lambda: loss_backward(m, c, est), a.reps)
        ws = int(blib.fsem_bsssdr_workspace_bytes(B, L))
        rec = {
            "scores_ms_per_call": round(ms_f, 4),
            "differentiable_scores_ms_per_call": round(ms_d, 4),
            "loss_backward_ms_per_call": round(ms_fb, 4),
            "loss_backward_over_scores": round(ms_fb / ms_f, 3),
            "rows_per_s_loss_backward": round(B / ms_fb * 1e3, 1),
            "state_bytes_per_row": int(lib.fsem_bsssdr_state_floats(B, L)) * 4 // B,
            "state_bytes_per_row_beyond_the_forward_workspace": (int(lib.fsem_bsssdr_state_floats(B, L)) * 4 - ws) // B,
        }
        print(shape, json.dumps(rec), flush=True)
        Bt = min(B, a.torch_batch)
        g_eng = loss_backward(m, c[:Bt], n[:Bt].clone().requires_grad_(True)).double()
        for name, dt in (("torch_float64", torch.float64), ("torch_float32", torch.float32)):
            ht = n[:Bt].to(dt).requires_grad_(True)

            def fb():
                ht.grad = None
                torch_loss(c[:Bt], ht, dt).backward()
                return ht.grad

            try:
                with torch.no_grad():
                    ms_tf = median_ms(lambda: torch_loss(c[:Bt], ht, dt), a.torch_reps, warm=1)
                ms_tfb = median_ms(fb, a.torch_reps, warm=1)
                grad = fb().double()
            except RuntimeError as e:   # (a system that is singular in this dtype)
                rec[name] = {"rows_timed": Bt, "failed": str(e).splitlines()[0][:120]}
                continue
            if dt == torch.float64:
                grad64 = grad
                scale = grad64.abs().amax(1, keepdim=True).clamp_min(1e-300)
                rec["engine_gradient_error_against_float64"] = float(((g_eng - grad64).abs() / scale).max())
            else:
                rec["torch_float32_gradient_error_against_float64"] = float(((grad - grad64).abs() / scale).max())
            rec[name] = {"rows_timed": Bt, "forward_ms_scaled_to_batch": round(ms_tf * B / Bt, 3),
                         "forward_backward_ms_scaled_to_batch": round(ms_tfb * B / Bt, 3),
                         "engine_speedup_forward_backward": round(ms_tfb * B / Bt / ms_fb, 2)}
            del ht, grad
        out["shapes"][shape] = rec
        del c, n, est
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
