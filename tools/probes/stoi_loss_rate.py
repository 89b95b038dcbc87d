"""Rate of STOI.loss + backward (csrc/stoi_grad.hip) beside STOI.scores on the same rows (the forward alone) and
beside the same definition written in torch ops on the same device tensors with autograd -- float64 (the
reference) and float32 (what a training script would write, with its gradient error against float64).  HIP
events, 3 warm-up calls, the median of ``--reps`` calls.  Shapes: B x L at 16 kHz, by default 64 x 4 s and the
bench's headline shape 4096 x 10 s.  The torch formulation materialises each row's [S, 15, 30] segments and
selects frames row by row: it runs on the first ``--torch-batch`` rows and its times are scaled to the batch.

    python tools/probes/stoi_loss_rate.py [--reps 20] [--out profiles/stoi_loss_a/stoi_loss_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import STOI, _native  # noqa: E402
from fast_speech_enhancement_metrics_amd.resample import sinc_kernel  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402


def definition(x, y, sr: int, dtype):
    """(stoi, estoi) 0-d tensors of one row pair at rate sr in ``dtype`` on the rows' device, or None without
    a 30-frame segment: resampler, frame selection by the clean row, overlap-add, STFT, band envelopes with
    the subgradient 0 at 0, segments, both correlations (include/fsem.h, "STOI with gradients")."""
    dev = x.device
    kern, width, orig, new = sinc_kernel(sr, 10000)
    kern = kern.to(dev, dtype)

    def to10k(v):
        g = torch.nn.functional.pad(v.to(dtype), (width, width + orig)).unfold(0, kern.shape[1], orig)
        return (g @ kern.T).reshape(-1)[:-(-new * v.numel() // orig)]

    x10, y10 = to10k(x.detach()), to10k(y)
    w = torch.hann_window(257, device=dev)[1:].to(dtype)
    e = 20 * torch.log10((x10.unfold(0, 256, 128) * w).norm(dim=1) + 1e-9)
    keep = (e.max() - 40 - e) < 0
    S = int(keep.sum()) - 31
    if S <= 0:
        return None
    freqs = torch.arange(257, dtype=torch.float64) * (5000.0 / 256)
    obm = torch.zeros(15, 257, dtype=dtype)
    for i in range(15):
        lo, hi = 150 * 2.0 ** ((2 * i - 1) / 6), 150 * 2.0 ** ((2 * i + 1) / 6)
        obm[i, int((freqs - lo).abs().argmin()):int((freqs - hi).abs().argmin())] = 1
    obm = obm.to(dev)

    def envelopes(v):
        k = (v.unfold(0, 256, 128) * w)[keep]
        z = torch.zeros(1, 128, dtype=dtype, device=dev)
        sig = (torch.cat([k[:, :128], z]) + torch.cat([z, k[:, 128:]])).reshape(-1)
        fr = sig.unfold(0, 512, 128)[:, 128:384] * w
        p = torch.fft.rfft(torch.nn.functional.pad(fr, (128, 128)), dim=1).abs().square() @ obm.T
        pos = p > 0
        return (torch.where(pos, p, torch.ones_like(p)).sqrt() * pos).T

    xs = envelopes(x10).unfold(1, 30, 1)[:, :S].transpose(0, 1)
    ys = envelopes(y10).unfold(1, 30, 1)[:, :S].transpose(0, 1)

    def unit(v):
        v = v - v.mean(dim=2, keepdim=True)
        return v / torch.sqrt(v.square().sum(dim=2, keepdim=True) + 30e-24)

    def unit2(v):
        c = v - v.mean(dim=2, keepdim=True)
        n2 = c.square().sum(dim=2, keepdim=True) + 30e-24
        a = c / n2.sqrt()
        a = a - a.mean(dim=1, keepdim=True)
        return a / torch.sqrt(a.square().sum(dim=1, keepdim=True) + (14 / 15) * (1e-24 / n2).sum(dim=1, keepdim=True)
                              + 15e-24)

    nx = torch.linalg.vector_norm(xs, dim=2, keepdim=True)
    ny = torch.linalg.vector_norm(ys, dim=2, keepdim=True)
    yc = torch.minimum(ys * (nx / (ny + 1e-9)), xs * (1 + 10 ** (15 / 20)))
    return (unit(xs) * unit(yc)).sum() / 15 / S, (unit2(xs) * unit2(ys)).sum() / 30 / S


def torch_loss(c, est, sr: int, dtype):
    """-mean ESTOI over the scored rows, the definition row by row."""
    vals = [definition(c[b], est[b], sr, dtype) for b in range(c.shape[0])]
    vals = [v[1] for v in vals if v is not None]
    return -torch.stack(vals).mean()


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


def loss_backward(m, c, est, sr):
    est.grad = None
    m.loss(c, est, sr, key="ESTOI").backward()
    return est.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "stoi_loss_a", "stoi_loss_rate.json"))
    ap.add_argument("--shapes", default="64x64000,4096x160000")
    a = ap.parse_args()
    sr = 16000
    m = STOI(sr, use_gpu=True)
    lib = _native.load()
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, sr, seed=42, device="cuda")
        est = n.clone().requires_grad_(True)
        ms_f = median_ms(lambda: m.scores(c, n, sr), a.reps)
        with torch.no_grad():
            ms_d = median_ms(lambda: m.differentiable_scores(c, n, sr), a.reps)
        ms_fb = median_ms(lambda: loss_backward(m, c, est, sr), a.reps)
        rec = {
            "scores_ms_per_call": round(ms_f, 4),
            "differentiable_scores_ms_per_call": round(ms_d, 4),
            "loss_backward_ms_per_call": round(ms_fb, 4),
            "loss_backward_over_scores": round(ms_fb / ms_f, 3),
            "rows_per_s_loss_backward": round(B / ms_fb * 1e3, 1),
            "state_bytes_per_row": int(lib.fsem_stoi_state_floats(B, L, sr)) * 4 // B,
            "workspace_bytes_per_row": int(lib.fsem_stoi_workspace_bytes(B, L, sr)) // B,
        }
        Bt = min(B, a.torch_batch)
        g_eng = loss_backward(m, c[:Bt], n[:Bt].clone().requires_grad_(True), sr).double()
        for name, dt in (("torch_float64", torch.float64), ("torch_float32", torch.float32)):
            ht = n[:Bt].to(dt).requires_grad_(True)

            def fb():
                ht.grad = None
                torch_loss(c[:Bt], ht, sr, dt).backward()
                return ht.grad

            with torch.no_grad():
                ms_tf = median_ms(lambda: torch_loss(c[:Bt], ht, sr, dt), a.torch_reps, warm=1)
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
