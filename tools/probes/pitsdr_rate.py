"""Rate of PITSDR.scores and of PITSDR.loss + backward (csrc/pitsdr.hip) beside the written definition in
torch ops on the same device tensors -- float64 (the exact reference, forward and backward) and float32
(what a training script writes, with its error against float64) -- and, at S = E = 1, beside SDR.scores on
the same rows.  HIP events, 3 warm-up calls, the median of ``--reps`` calls.  The engine's bytes (forward:
every row read once; backward: every row read once, the gradient written once) are set against torch's
device-to-device copy of the same size measured in the same process (bytes read + written) and against
sdr_rate.py's 6.29 TB/s float4 copy.  Shapes: B x S x E x L, by default the bench's headline
shape as two-source mixtures (4096 x 2 x 2 x 160000 at 16 kHz) and the reference's benchmark setting
(64 x 2 x 2 x 256000).  The torch formulations keep [B, S, E, L] temporaries: they run on the first
``--torch-batch`` mixtures and their times are scaled to the whole batch.

    python tools/probes/pitsdr_rate.py [--reps 20] [--out profiles/pitsdr_a/pitsdr_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import PITSDR, SDR  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402


COPY_BW = 6.29e12  # the float4 copy of tools/probes/sdr_rate.py, bytes/s (torch's own copy_ is measured beside it)


def definition(s: torch.Tensor, h: torch.Tensor):
    """(si_mat, snr_mat) [B, S, E] in the dtype of the inputs: the definition in torch ops."""
    d = h[:, None] - s[:, :, None]
    ss, hh = s.square().sum(2)[:, :, None], h.square().sum(2)[:, None, :]
    sh = torch.einsum("bil,bel->bie", s, h)
    snr = 10 * torch.log10(ss / d.square().sum(3))
    t = sh * sh / ss
    return 10 * torch.log10(t / (hh - t).clamp_min(0)), snr


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


def copy_bandwidth(nbytes: int, reps: int) -> float:
    """bytes/s (read + written) of a device-to-device copy of nbytes of float32."""
    n = max(nbytes // 4 // 4 * 4, 1 << 20)
    a = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
    b = torch.empty_like(a)
    ms = median_ms(lambda: b.copy_(a), reps)
    return 2 * n * 4 / (ms * 1e-3)


def mixtures(B: int, S: int, L: int, sr: int):
    """(sources, estimates) [B, S, L] on the device: estimate e is the noisy version of source e."""
    cs, ns = [], []
    for k in range(S):  # (one slice of B rows at a time bounds the generator's temporaries)
        c, n, _ = speech_like_pairs(B, L, sr, seed=42 + k, device="cuda", snr_low=-5, snr_high=40)
        cs.append(c)
        ns.append(n)
    return torch.stack(cs, 1).contiguous(), torch.stack(ns, 1).contiguous()


def loss_backward(m, s, est):
    est.grad = None
    m.loss(s, est).backward()
    return est.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "pitsdr_a", "pitsdr_rate.json"))
    ap.add_argument("--shapes", default="4096x2x2x160000,64x2x2x256000")
    a = ap.parse_args()
    sr = 16000
    m = PITSDR(sr, use_gpu=True)
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, S, E, L = (int(v) for v in shape.split("x"))
        s, h = mixtures(B, S, L, sr)
        h = h[:, :E].contiguous()
        est = h.clone().requires_grad_(True)
        fwd_bytes = (S + E) * B * L * 4
        bwd_bytes = (S + 2 * E) * B * L * 4
        copy = copy_bandwidth(fwd_bytes, a.reps)
        ms_f = median_ms(lambda: m.scores(s, h), a.reps)
        ms_fb = median_ms(lambda: loss_backward(m, s, est), a.reps)
        rec = {
            "copy_TB_per_s_same_process": round(copy / 1e12, 3),
            "scores": {"ms_per_call": round(ms_f, 4), "mixtures_per_s": round(B / ms_f * 1e3, 1),
                       "bytes": fwd_bytes, "TB_per_s": round(fwd_bytes / ms_f / 1e9, 3),
                       "share_of_copy": round(fwd_bytes / (ms_f * 1e-3) / copy, 4),
                       "share_of_6.29TBps_copy": round(fwd_bytes / (ms_f * 1e-3) / COPY_BW, 4)},
            "loss_backward": {"ms_per_call": round(ms_fb, 4), "bytes": fwd_bytes + bwd_bytes,
                              "TB_per_s": round((fwd_bytes + bwd_bytes) / ms_fb / 1e9, 3),
                              "share_of_copy": round((fwd_bytes + bwd_bytes) / (ms_fb * 1e-3) / copy, 4),
                              "share_of_6.29TBps_copy": round((fwd_bytes + bwd_bytes) / (ms_fb * 1e-3) / COPY_BW, 4)},
        }
        # the definition in torch ops on the first Bt mixtures, scaled to B
        Bt = min(B, a.torch_batch)
        eng_si, eng_snr, perm, si_mat, snr_mat = m.scores(s[:Bt], h[:Bt], return_matrix=True)
        g_eng = loss_backward(m, s[:Bt], est[:Bt].detach().clone().requires_grad_(True))
        idx = perm.long()[:, None, :]
        for name, dt in (("torch_float64", torch.float64), ("torch_float32", torch.float32)):
            st, ht = s[:Bt].to(dt), h[:Bt].to(dt).requires_grad_(True)

            def fb():
                ht.grad = None
                (-definition(st, ht)[0].gather(1, idx)[:, 0].mean()).backward()
                return ht.grad

            with torch.no_grad():
                ms_tf = median_ms(lambda: definition(st, ht), a.torch_reps, warm=1)
                ref = definition(st, ht)
            ms_tfb = median_ms(fb, a.torch_reps, warm=1)
            grad = fb()
            if dt == torch.float64:
                ref64, grad64 = ref, grad
                rec["engine_error_against_float64"] = {
                    "SI-SDR_dB": float((si_mat.double() - ref[0]).abs().max()),
                    "SNR_dB": float((snr_mat.double() - ref[1]).abs().max()),
                    "gradient_relative_to_largest": float((g_eng.double() - grad).abs().max() / grad.abs().max())}
            else:
                rec["torch_float32_error_against_float64"] = {
                    "SI-SDR_dB": float((ref[0].double() - ref64[0]).abs().max()),
                    "SNR_dB": float((ref[1].double() - ref64[1]).abs().max()),
                    "gradient_relative_to_largest": float((grad.double() - grad64).abs().max() / grad64.abs().max())}
            rec[name] = {"mixtures_timed": Bt, "forward_ms_scaled_to_batch": round(ms_tf * B / Bt, 3),
                         "forward_backward_ms_scaled_to_batch": round(ms_tfb * B / Bt, 3),
                         "engine_speedup_forward": round(ms_tf * B / Bt / ms_f, 2),
                         "engine_speedup_forward_backward": round(ms_tfb * B / Bt / ms_fb, 2)}
            del st, ht, ref, grad
        del ref64, grad64
        # S = E = 1 beside SDR.scores on the same rows
        c1, n1 = s[:, 0], h[:, 0]
        sdr = SDR(sr, use_gpu=True)
        ms_p1 = median_ms(lambda: m.scores(c1, n1), a.reps)
        ms_s1 = median_ms(lambda: sdr.scores(c1, n1), a.reps)
        rec["one_source"] = {"pitsdr_ms_per_call": round(ms_p1, 4), "sdr_ms_per_call": round(ms_s1, 4),
                             "pitsdr_share_of_copy": round(2 * B * L * 4 / (ms_p1 * 1e-3) / copy, 4),
                             "sdr_share_of_copy": round(2 * B * L * 4 / (ms_s1 * 1e-3) / copy, 4),
                             "worst_abs_SI-SDR_difference_dB": float(
                                 (m.scores(c1, n1)[0][:, 0].double() - sdr.scores(c1, n1)[0].double()).abs().max())}
        out["shapes"][shape] = rec
        del s, h, est
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
