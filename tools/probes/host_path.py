"""Host time per drop-in call metric(clean, noisy) of LSD and SDR at 64 x 16000 (the shape where host
overhead shows): python tools/probes/host_path.py ROOT TAG OUT.json
ROOT is the tree whose package is timed (this one, or a checkout of another commit with its libraries built): two
commits are compared by alternating processes in one session (profiles/host_path_a/host_path.json)."""
import json
import os
import statistics
import sys
import time

root, tag, out = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3]
sys.path.insert(0, root)

import torch  # noqa: E402

import fast_speech_enhancement_metrics_amd as pkg  # noqa: E402
from fast_speech_enhancement_metrics_amd import LSD, SDR, _build  # noqa: E402

assert os.path.dirname(os.path.abspath(pkg.__file__)).startswith(root), pkg.__file__
WARMUP, CALLS = 50, 400
g = torch.Generator().manual_seed(3)
clean = (torch.randn(64, 16000, generator=g) * 0.1).cuda()
noisy = clean + 0.03 * torch.randn(64, 16000, generator=g).cuda()
rec = {"tag": tag, "package": os.path.dirname(pkg.__file__), "build_id": _build.source_hash(), "shape": [64, 16000],
       "warmup": WARMUP, "calls": CALLS, "unit": "us per call (host clock around the call; the call ends in the "
       "scores' copy to the host)"}
for cls in (LSD, SDR):
    m = cls(16000, use_gpu=True)
    for _ in range(WARMUP):
        res = m(clean, noisy)
    torch.cuda.synchronize()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        res = m(clean, noisy)
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    rec[cls.__name__] = {"median": statistics.median(ts), "p10": ts[CALLS // 10], "p90": ts[CALLS * 9 // 10],
                         "min": ts[0], "first_row": res[0]}
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps(rec))
