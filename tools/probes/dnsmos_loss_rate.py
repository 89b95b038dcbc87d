"""Rate of DNSMOS.loss + backward (csrc/dnsmos_grad.hip) beside DNSMOS.scores on the same rows (the forward
alone), and beside the package's torch formulation (``_cpu.dnsmos_features`` in float32, ``_cpu.dnsmos_network``
under float16 autocast) with autograd on the same device, on the first ``--torch-batch`` rows, scaled to the batch.
HIP events, warm-up calls, the median of ``--reps`` calls.  Shapes: B x L at 16 kHz, by default 4096 x 10 s and
64 x 16 s.

With ``--parent-lib`` (a libfsem_dnsmos.so built from the parent commit) it also times ``fsem_dnsmos_f32`` through
this build's library and the parent's in turn, ``--ab-runs`` times each, through the same ctypes calls: what moving
the forward's kernels into fsem_dnsmos_kernels.h cost, beside the parent's own run-to-run spread.

    python tools/probes/dnsmos_loss_rate.py [--reps 5] [--out profiles/dnsmos_loss_a/dnsmos_loss_rate.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from fast_speech_enhancement_metrics_amd import DNSMOS, _cpu, _native  # noqa: E402
from fast_speech_enhancement_metrics_amd.DNSMOS import WEIGHT_SHAPES  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def median_ms(fn, reps: int, warm: int = 2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return statistics.median(timed(fn)[0] for _ in range(reps))


def loss_backward(m, est):
    est.grad = None
    m.loss(est).backward()
    return est.grad


def torch_loss(w, rows):
    """-mean OVRL of full 16 kHz rows [B, L >= 144160] in the package's torch ops, the network under float16 autocast."""
    c0, c1, c2 = (torch.tensor(c, device=rows.device)[2] for c in _cpu._DNSMOS_POLY)
    total = 0.0
    for b in range(rows.shape[0]):
        segs = rows[b].unfold(0, _cpu.DNSMOS_SEGMENT, _cpu.DNSMOS_HOP)
        image = _cpu.dnsmos_features(w, segs)
        with torch.autocast("cuda", dtype=torch.float16):
            raw = _cpu.dnsmos_network(w, image)[:, 2].float()
        total = total + (c0 + c1 * raw + c2 * raw.square()).mean()
    return -total / rows.shape[0]


class RawLibrary:
    """fsem_dnsmos_f32 of one libfsem_dnsmos.so through ctypes, with its own packed weights."""

    def __init__(self, path, weights, device):
        self.lib = ctypes.CDLL(path)
        for name, (restype, argtypes) in _native.DNSMOS_SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        dev = [weights[k].to(device) for k in WEIGHT_SHAPES]
        ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        self.blob = torch.empty(self.lib.fsem_dnsmos_weights_bytes(), dtype=torch.uint8, device=device)
        rc = self.lib.fsem_dnsmos_pack_weights_f32(ptrs, self.blob.data_ptr(), self.blob.numel(),
                                                   _native.stream_handle(device))
        assert rc == 0, rc
        torch.cuda.synchronize()

    def scores(self, rows):
        B, L = rows.shape
        out = torch.empty(B, 3, device=rows.device)
        ws = _native.workspace(self.lib.fsem_dnsmos_workspace_bytes(B, L), rows.device)
        rc = self.lib.fsem_dnsmos_f32(rows.data_ptr(), B, L, rows.stride(0), None, self.blob.data_ptr(), out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _native.stream_handle(rows.device))
        assert rc == 0, rc
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "dnsmos_loss_a", "dnsmos_loss_rate.json"))
    ap.add_argument("--shapes", default="4096x160000,64x256000")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    a = ap.parse_args()
    sr = 16000
    m = DNSMOS(sr, use_gpu=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    w_dev = {k: v.to(dev) for k, v in m.weights.items()}
    lib = _native.load()
    out = {"sample_rate": sr, "reps": a.reps, "torch_reps": a.torch_reps, "shapes": {}}
    new_lib = RawLibrary(_native.DNSMOS_LIB_PATH, m.weights, dev)
    old_lib = RawLibrary(a.parent_lib, m.weights, dev) if a.parent_lib else None
    for shape in a.shapes.split(","):
        B, L = (int(v) for v in shape.split("x"))
        _, n, _ = speech_like_pairs(B, L, sr, device="cuda", snr_low=-5, snr_high=40)
        est = n.clone().requires_grad_(True)
        segments = B * int(_native.load_dnsmos().fsem_dnsmos_segments(L))
        ms_f = median_ms(lambda: m.scores(n), a.reps)
        ms_fb = median_ms(lambda: loss_backward(m, est), a.reps)
        rec = {
            "segments": segments,
            "scores_ms_per_call": round(ms_f, 3),
            "loss_backward_ms_per_call": round(ms_fb, 3),
            "loss_backward_over_scores": round(ms_fb / ms_f, 3),
            "rows_per_s_loss_backward": round(B / ms_fb * 1e3, 1),
            "scratch_bytes": int(lib.fsem_dnsmos_grad_scratch_floats(B, L, 16)) * 4,
        }
        print(shape, json.dumps(rec), flush=True)
        if old_lib is not None:
            assert torch.equal(new_lib.scores(n).view(torch.int32), old_lib.scores(n).view(torch.int32))
            rec["scores_bitwise_equal_to_parent"] = True
            runs = []
            for run in range(a.ab_runs):
                for name, rl in (("parent", old_lib), ("new", new_lib)):
                    runs.append({"build": name, "run": run + 1,
                                 "ms_per_call": round(median_ms(lambda: rl.scores(n), a.reps, warm=1), 3)})
            rec["fsem_dnsmos_f32_parent_and_new_alternating"] = runs
            print(shape, json.dumps(runs), flush=True)
        Bt = min(B, a.torch_batch)
        if Bt < 1:   # (--torch-batch 0: the engine alone)
            out["shapes"][shape] = rec
            continue
        ht = n[:Bt].clone().requires_grad_(True)

        def fb():
            ht.grad = None
            torch_loss(w_dev, ht).backward()
            return ht.grad

        try:
            ms_tfb = median_ms(fb, a.torch_reps, warm=1)
            finite = bool(torch.isfinite(fb()).all())
            rec["torch_float16_autocast"] = {"rows_timed": Bt, "gradient_finite": finite,
                                             "forward_backward_ms_scaled_to_batch": round(ms_tfb * B / Bt, 2),
                                             "engine_speedup_forward_backward": round(ms_tfb * B / Bt / ms_fb, 2)}
        except RuntimeError as e:
            rec["torch_float16_autocast"] = {"rows_timed": Bt, "failed": str(e).splitlines()[0][:160]}
        print(shape, json.dumps(rec["torch_float16_autocast"]), flush=True)
        out["shapes"][shape] = rec
        del n, est, ht
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
