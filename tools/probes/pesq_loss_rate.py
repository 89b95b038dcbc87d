"""Rate of PESQ.loss + backward (csrc/pesq_grad.hip) beside PESQ.scores on the same rows (the forward alone) and
beside the same definition written in torch ops on the same device tensors with autograd -- float64 (the
reference) and float32 (what a training script would write, with its gradient error against float64).  HIP
events, 3 warm-up calls, the median of ``--reps`` calls.  Shapes: B x L at 16 kHz, by default 64 x 16 s and the
bench's headline shape 4096 x 10 s.  The torch formulation runs on the first ``--torch-batch`` rows and its
times are scaled to the batch; its two IIRs are convolutions with the filters' impulse responses cut at 4096
taps (both have decayed below 1e-11 of their peak within 832), by FFT in the formulation's dtype.  The
engine's forward and backward entries are also timed on their own (``--no-torch`` stops there, for a kernel
trace of the engine alone).

    python tools/probes/pesq_loss_rate.py [--reps 20] [--out profiles/pesq_loss_a/pesq_loss_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
from scipy.signal import lfilter, sosfilt

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import PESQ, _cpu, _native  # noqa: E402
from fast_speech_enhancement_metrics_amd import _tables as T  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402

TAPS = 4096
ALPHA = (1.0, 0.3, 0.1, 0.03)   # denoised = clean + alpha (noisy - clean): scores spread over the scale


def _impulse_responses():
    d = np.zeros(TAPS)
    d[0] = 1.0
    return (torch.from_numpy(sosfilt(_cpu._BP_SOS, d)), torch.from_numpy(lfilter(_cpu._PRE_B, _cpu._PRE_A, d)))


def definition(c, x, dtype, consts):
    """(mos, sym, asym) [B] of row pairs [B, L] in ``dtype`` on the rows' device (include/fsem.h, "PESQ with
    gradients"), every decision a constant, the subgradient 0 at a zero symmetric disturbance."""
    h_bp, h_pre, thr, ex, wb, corr, fbank = consts
    B, L = x.shape
    n_fft = 1 << (L + TAPS).bit_length()

    def fir(v, h):
        return torch.fft.irfft(torch.fft.rfft(v, n_fft) * torch.fft.rfft(h, n_fft), n_fft)[:, :L]

    w = torch.ones(L, dtype=dtype, device=x.device)
    w[:15] = torch.arange(1, 16, dtype=dtype, device=x.device) / 16
    w[-15:] = torch.arange(15, 0, -1, dtype=dtype, device=x.device) / 16
    hann = torch.hann_window(512, dtype=dtype, device=x.device)

    def bark(v):
        u = fir(v, h_bp)
        s = v * torch.sqrt(1e7 / ((u * u).sum(1, keepdim=True) / (L + 5120) / 1.04684))
        s = torch.nn.functional.pad(fir(s * w, h_pre), (0, L % 256))
        z = torch.fft.rfft(s.unfold(1, 512, 256) * hann, dim=2)
        p = (z.real.square() + z.imag.square())[:, :, :256]
        return (p @ fbank.T) * corr   # [B, F, 49]; fbank's column 0 (the DC bin) is zero

    with torch.no_grad():
        cb = bark(c.to(dtype))
    nb = bark(x.to(dtype))
    sil = (cb * (cb > 100 * thr)).sum(2) < 1e7
    keep = (~sil)[:, :, None]
    mc = (cb * ((cb > 100 * thr) & keep)).mean(1)
    mn = (nb * ((nb > 100 * thr) & keep)).mean(1)
    ec = ((mn + 1000) / (mc + 1000)).clamp(0.01, 100)[:, None] * cb
    fr = ((ec * (ec > thr)).sum(2) + 5e3) / ((nb * (nb > thr)).sum(2) + 5e3)
    fr = torch.cat([fr[:, :1], 0.8 * fr[:, 1:] + 0.2 * fr[:, :-1]], 1).clamp(3e-4, 5.0)
    en = fr[:, :, None] * nb

    def loud(p):
        v = (2 * thr) ** ex * ((0.5 + 0.5 * p / thr) ** ex - 1)
        return torch.where(p <= thr, torch.zeros_like(v), v) * T.SL_16K

    lc, ln = loud(ec), loud(en)
    d = ln - lc
    d = d.sign() * (d.abs() - 0.25 * torch.minimum(lc, ln)).clamp(min=0)
    s2 = ((wb * d)[:, :, 1:] ** 2).sum(2)
    pos = s2 > 0
    sym = (float(wb[1:].double().sum()) ** 0.5 * torch.where(pos, s2, torch.ones_like(s2)).sqrt() * pos).clamp(min=1e-20)
    a = ((en + 50) / (ec + 50)) ** 1.2
    a = torch.where(a < 3, torch.zeros_like(a), a).clamp(max=12)
    asym = (wb * d * a)[:, :, 1:].abs().sum(2).clamp(min=1e-20)
    fw = (((ec * (ec > thr)).sum(2) + 1e5) / 1e7) ** 0.04
    sym, asym = (sym / fw).clamp(max=45), (asym / fw).clamp(max=45)

    def pool(v):
        return (v.unfold(1, 20, 10) ** 6).mean(2).pow(1 / 6).square().mean(1).sqrt()

    sd, ad = pool(sym), pool(asym)
    m = 4.5 - 0.1 * sd - 0.0309 * ad
    return 0.999 + 4 / (1 + torch.exp(-1.3669 * m + 3.8224)), sd, ad


def constants(dtype, dev):
    h_bp, h_pre = _impulse_responses()
    edges = np.concatenate([[0], np.cumsum(T.BINS_PER_BAND)])
    fbank = torch.zeros(49, 256, dtype=torch.float64)
    for i in range(49):
        fbank[i, max(int(edges[i]), 1):int(edges[i + 1])] = 1.0
    vals = (h_bp, h_pre, torch.tensor(T.ABS_THRESH_POWER, dtype=torch.float64),
            (6 / (torch.tensor(T.CENTRE_BARK) + 2.0)).clamp(1.0, 2.0) ** 0.15 * T.ZWICKER_POWER,
            torch.tensor(T.WIDTH_BARK, dtype=torch.float64),
            torch.tensor(T.POW_DENS_CORRECTION, dtype=torch.float64) * T.SP_16K, fbank)
    return tuple(v.to(dev, dtype) for v in vals)


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
    m.loss(c, est, key="PESQ").backward()
    return est.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-batch", type=int, default=8)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "pesq_loss_a", "pesq_loss_rate.json"))
    ap.add_argument("--shapes", default="64x256000,4096x160000")
    a = ap.parse_args()
    m = PESQ(16000, use_gpu=True)
    lib = _native.load()
    out = {"sample_rate": 16000, "reps": a.reps, "torch_reps": a.torch_reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        c, n, _ = speech_like_pairs(B, L, 16000, seed=42, device="cuda")
        alpha = torch.tensor(ALPHA, device="cuda").repeat((B + 3) // 4)[:B, None]
        n = c + alpha * (n - c)
        est = n.clone().requires_grad_(True)
        ms_f = median_ms(lambda: m.scores(c, n), a.reps)
        with torch.no_grad():
            ms_d = median_ms(lambda: m.differentiable_scores(c, n), a.reps)
        ms_fb = median_ms(lambda: loss_backward(m, c, est), a.reps)
        # the two entries on their own
        mos = torch.empty(B, device="cuda")
        dist = torch.empty(2, B, device="cuda")
        grad = torch.empty(B, L, device="cuda")
        ones = torch.ones(B, device="cuda")
        state = torch.empty(lib.fsem_pesq_state_floats(B, L), device="cuda")
        st = _native.stream_handle(c.device)
        ms_state = median_ms(lambda: _native.check(lib.fsem_pesq_state_f32(
            c.data_ptr(), n.data_ptr(), B, L, L, None, mos.data_ptr(), dist.data_ptr(), state.data_ptr(), st), "state"),
            a.reps)
        ms_grad = median_ms(lambda: _native.check(lib.fsem_pesq_grad_f32(
            n.data_ptr(), B, L, L, None, state.data_ptr(), ones.data_ptr(), None, None, grad.data_ptr(), L, st), "grad"),
            a.reps)
        del state, grad
        rec = {
            "scores_ms_per_call": round(ms_f, 4),
            "differentiable_scores_ms_per_call": round(ms_d, 4),
            "loss_backward_ms_per_call": round(ms_fb, 4),
            "loss_backward_over_scores": round(ms_fb / ms_f, 3),
            "state_entry_ms": round(ms_state, 4),
            "grad_entry_ms": round(ms_grad, 4),
            "rows_per_s_loss_backward": round(B / ms_fb * 1e3, 1),
            "state_bytes_per_row": int(lib.fsem_pesq_state_floats(B, L)) * 4 // B,
            "workspace_bytes_per_row": int(lib.fsem_pesq_workspace_bytes(B, L)) // B,
        }
        Bt = min(B, a.torch_batch)
        if not a.no_torch:
            g_eng = loss_backward(m, c[:Bt], n[:Bt].clone().requires_grad_(True)).double()
            for name, dt in (("torch_float64", torch.float64), ("torch_float32", torch.float32)):
                consts = constants(dt, c.device)
                ht = n[:Bt].to(dt).requires_grad_(True)

                def fb():
                    ht.grad = None
                    (-definition(c[:Bt], ht, dt, consts)[0].mean()).backward()
                    return ht.grad

                with torch.no_grad():
                    ms_tf = median_ms(lambda: definition(c[:Bt], ht, dt, consts), a.torch_reps, warm=1)
                ms_tfb = median_ms(fb, a.torch_reps, warm=1)
                g = fb().double()
                if dt == torch.float64:
                    grad64 = g
                    scale = grad64.abs().amax(1, keepdim=True).clamp_min(1e-300)
                    rec["engine_gradient_error_against_float64"] = float(((g_eng - grad64).abs() / scale).max())
                else:
                    rec["torch_float32_gradient_error_against_float64"] = float(((g - grad64).abs() / scale).max())
                rec[name] = {"rows_timed": Bt, "forward_ms_scaled_to_batch": round(ms_tf * B / Bt, 3),
                             "forward_backward_ms_scaled_to_batch": round(ms_tfb * B / Bt, 3),
                             "engine_speedup_forward_backward": round(ms_tfb * B / Bt / ms_fb, 2)}
                del ht, g
            del grad64
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
