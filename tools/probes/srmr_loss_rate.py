"""Rate of SRMR.loss + backward (csrc/srmr_grad.hip) beside SRMR.scores on the same rows (the forward alone),
with the backward's scratch bytes per row and rows per pass.  HIP events, 3 warm-up calls, the median of
``--reps`` calls.  Shapes: B x L at 16 kHz, by default the bench's headline shape 4096 x 10 s and 64 x 16 s.

``--parent-lib PATH`` (a libfsem.so built from the parent commit): fsem_srmr_f32 of that library and of this
tree's, alternating call by call on the same rows in the same visit, the median of each -- what moving the
shared code into fsem_srmr_kernels.h cost the forward.

    python tools/probes/srmr_loss_rate.py [--reps 10] [--parent-lib PATH] [--out profiles/srmr_loss_a/srmr_loss_rate.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import SRMR, _native  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402


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


def loss_backward(m, est):
    est.grad = None
    m.loss(est).backward()
    return est.grad


def forward_call(lib, rows, sr):
    """One fsem_srmr_f32 call of ``lib`` on the rows, (scores, energies)."""
    B, L = rows.shape
    out = torch.empty(B, dtype=torch.float32, device=rows.device)
    energies = torch.empty(B, 23, 8, dtype=torch.float64, device=rows.device)
    rc = lib.fsem_srmr_f32(rows.data_ptr(), B, L, rows.stride(0), None, sr, energies.data_ptr(), out.data_ptr(),
                           _native.stream_handle(rows.device))
    assert rc == 0
    return out, energies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "srmr_loss_a", "srmr_loss_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    a = ap.parse_args()
    sr = 16000
    m = SRMR(sr, use_gpu=True)
    lib = _native.load()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib, mode=ctypes.RTLD_LOCAL)
        parent.fsem_srmr_f32.restype, parent.fsem_srmr_f32.argtypes = _native.SIGNATURES["fsem_srmr_f32"]
    out = {"sample_rate": sr, "reps": a.reps, "shapes": {}}
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        _, n, _ = speech_like_pairs(B, L, sr, seed=42, device="cuda")
        est = n.clone().requires_grad_(True)
        ms_f = median_ms(lambda: m.scores(n), a.reps)
        with torch.no_grad():
            ms_d = median_ms(lambda: m.differentiable_scores(n), a.reps)
        ms_fb = median_ms(lambda: loss_backward(m, est), a.reps)
        grad = loss_backward(m, est)
        rec = {
            "scores_ms_per_call": round(ms_f, 4),
            "differentiable_scores_ms_per_call": round(ms_d, 4),
            "loss_backward_ms_per_call": round(ms_fb, 4),
            "loss_backward_over_scores": round(ms_fb / ms_f, 3),
            "rows_per_s_loss_backward": round(B / ms_fb * 1e3, 1),
            "backward_scratch_bytes": int(lib.fsem_srmrgrad_scratch_bytes(B, L)),
            "backward_scratch_bytes_per_row_of_a_pass": int(lib.fsem_srmrgrad_scratch_bytes(B, L))
            // min(B, int(lib.fsem_srmrgrad_pass_rows(L))),
            "rows_per_pass": int(lib.fsem_srmrgrad_pass_rows(L)),
            "state_bytes_kept_by_the_forward_per_row": 23 * 8 * 8,
            "gradient_finite": bool(torch.isfinite(grad).all()),
        }
        if parent is not None:
            for _ in range(3):
                forward_call(parent, n, sr), forward_call(lib, n, sr)
            torch.cuda.synchronize()
            t_old, t_new = [], []
            for _ in range(a.reps):
                t_old.append(timed(lambda: forward_call(parent, n, sr))[0])
                t_new.append(timed(lambda: forward_call(lib, n, sr))[0])
            same = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32),
                                   y.view(torch.int64) if y.dtype == torch.float64 else y.view(torch.int32))
                       for x, y in zip(forward_call(parent, n, sr), forward_call(lib, n, sr)))
            rec["forward_parent_library_ms"] = round(statistics.median(t_old), 4)
            rec["forward_this_library_ms"] = round(statistics.median(t_new), 4)
            rec["forward_bitwise_equal_to_parent"] = same
        out["shapes"][shape] = rec
        del n, est, grad
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
