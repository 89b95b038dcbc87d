"""Rate of LSD.loss + backward (csrc/lsd_grad.hip) beside LSD.scores on the same rows (the forward alone) and
beside the same definition written in torch ops on the same device tensors with autograd -- float64 (the
reference) and float32 (what a training script would write) -- with the gradient error of the engine and of
the float32 form against float64 (max over a row of |g - g_ref| / max|g_ref|, the worst row).  HIP events, 3
warm-up calls, the median of ``--reps`` calls.  Shapes: B x L at 16 kHz, by default the bench's headline shape
4096 x 10 s and 64 x 16 s.  The torch forms run on the first ``--torch-batch`` rows and their times are scaled to
the batch.

    python tools/probes/lsd_loss_rate.py [--reps 20] [--out profiles/lsd_loss_a/lsd_loss_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import LSD, _native  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402


def torch_loss(c, est, dtype):
    """mean LSD of 16 kHz rows [B, L] in ``dtype`` on the rows' device: the definition of include/fsem_lsd.h
    in torch ops (scale, centred 512-point STFT with hop 256 and a periodic Hann window, log ratio, root mean
    square over bins, mean over frames)."""
    s, h = c.to(dtype), est.to(dtype)
    a = (s * h).sum(1, keepdim=True) / (h.square().sum(1, keepdim=True) + 1e-8)
    w = torch.hann_window(512, dtype=dtype, device=s.device)
    S = torch.stft(s, 512, 256, window=w, center=True, pad_mode="constant", return_complex=True).abs()
    H = torch.stft(a * h, 512, 256, window=w, center=True, pad_mode="constant", return_complex=True).abs()
    return torch.log(S.square() / (H + 1e-8).square() + 1e-8).square().mean(1).sqrt().mean(1).mean()


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join("profiles", "lsd_loss_a", "lsd_loss_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    a = ap.parse_args()
    sr = 16000
    m = LSD(sr, use_gpu=True)
    lib, llib = _native.load(), _native.load_lsd()
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, seed=42, device="cuda")
        est = n.clone().requires_grad_(True)
        ms_f = median_ms(lambda: m.scores(c, n), a.reps)
        with torch.no_grad():
            ms_d = median_ms(lambda: m.differentiable_scores(c, n), a.reps)
        ms_fb = median_ms(lambda: loss_backward(m, c, est), a.reps)
        rec = {
            "scores_ms_per_call": round(ms_f, 4),
            "differentiable_scores_ms_per_call": round(ms_d, 4),
            "loss_backward_ms_per_call": round(ms_fb, 4),
            "loss_backward_over_scores": round(ms_fb / ms_f, 3),
            "rows_per_s_loss_backward": round(B / ms_fb * 1e3, 1),
            "backward_state_bytes_per_row": int(lib.fsem_lsd_grad_state_floats(B, L)) * 4 // B,
            "state_bytes_kept_by_the_forward": 0,
            "workspace_bytes_per_row": int(llib.fsem_lsd_workspace_bytes(B, L)) // B,
        }
        Bt = min(B, a.torch_batch)
        g_eng = loss_backward(m, c[:Bt], n[:Bt].clone().requires_grad_(True)).double()
        for name, dt in (("torch_float64", torch.float64), ("torch_float32", torch.float32)):
            ht = n[:Bt].to(dt).requires_grad_(True)

            def fb():
                ht.grad = None
                torch_loss(c[:Bt], ht, dt).backward()
                return ht.grad

            with torch.no_grad():
                ms_tf = median_ms(lambda: torch_loss(c[:Bt], ht, dt), a.torch_reps, warm=1)
            ms_tfb = median_ms(fb, a.torch_reps, warm=1)
            grad = fb().double()
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
        del c, n, est, grad64
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
