"""DNSMOS with gradients on the HIP engine (csrc/dnsmos_grad.hip) against the float64 gradient of
tests/dnsmos_grad_cases.py under twice the rounding emulation's own deviation (tests/golden/dnsmos_grad_basis.json):
the forward bitwise ``scores()``, the gradient on the fixture rows and keys, the image-gradient stage, segment
overlap, wraps and ragged batches, reproducibility (calls, batch position, ``ld``, pass size), non-finite rows, the
8 kHz path and ``loss``.  Rows are one or two segments; a test takes at most two segments of float64 reference."""
import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import DNSMOS, _native

from . import dnsmos_cases as dc
from . import dnsmos_grad_cases as gc
from .contract import assert_bitwise

pytestmark = pytest.mark.gpu

BAR = gc.MARGIN * gc.basis()["basis"]
BAR_IMAGE = gc.MARGIN * gc.basis()["basis_image"]
ONE_SEGMENT = 2500   # samples: 64 periods make 160000, one segment in which every sample feeds 57 or 58 positions


@pytest.fixture(scope="module")
def metric():
    return DNSMOS(16000, use_gpu=True, weights=dc.WEIGHTS)


def short_rows() -> torch.Tensor:
    """Three rows of ONE_SEGMENT samples with speech in them (row 1 of dnsmos_short is silent)."""
    src = dc.fixture("dnsmos_short").rows
    return torch.stack([src[0, :ONE_SEGMENT], src[0, 5000:5000 + ONE_SEGMENT], src[2, :ONE_SEGMENT]])


def engine(m, rows, g=None, lengths=None, sr=None):
    """(scores [B, 3], gradient [B, L]) float32 on the device for the upstream gradient g [3] or [B, 3] (OVRL alone)."""
    est = rows.cuda().requires_grad_(True)
    scores = m.differentiable_scores(est, sr, lengths=lengths)
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.shape == (rows.shape[0], 3)
    g = torch.tensor([0.0, 0.0, 1.0]) if g is None else torch.as_tensor(g, dtype=torch.float32)
    scores.backward(g.to(scores).expand_as(scores).where(torch.isfinite(scores), torch.zeros((), device="cuda")))
    assert est.grad.dtype == torch.float32 and est.grad.shape == rows.shape
    return scores.detach(), est.grad


def c_entry(m, rows, g, lengths=None, npass=16, ld_grad=None, image=False, want_raw=False):
    """fsem_dnsmos_grad_f32 (or the image stage) on CUDA rows [B, L] (any row stride) for g [B, 3]."""
    lib, dn = _native.load(), _native.load_dnsmos()
    B, L = rows.shape
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=rows.device)
    total = sum(dn.fsem_dnsmos_segments(int(k)) for k in (lengths if lengths is not None else [L] * B))
    g = torch.as_tensor(g, dtype=torch.float32).expand(B, 3).contiguous().cuda()
    scratch = torch.empty(lib.fsem_dnsmos_grad_scratch_floats(B, L, npass), dtype=torch.float32, device=rows.device)
    blob = m.grad_blob(rows.device)
    stream = _native.stream_handle(rows.device)
    if image:
        out = torch.full((total, 900, 161), 7.0, device=rows.device)
        rc = lib.fsem_dnsmos_grad_image_f32(rows.data_ptr(), B, L, rows.stride(0), _native.ptr(lens), blob.data_ptr(),
                                            g.data_ptr(), out.data_ptr(), scratch.data_ptr(), npass, stream)
        assert rc == _native.FSEM_OK, rc
        return out
    ld_grad = L if ld_grad is None else ld_grad
    grad = torch.full((B, ld_grad), 7.0, device=rows.device)
    raw = torch.full((total, 3), 7.0, device=rows.device) if want_raw else None
    rc = lib.fsem_dnsmos_grad_f32(rows.data_ptr(), B, L, rows.stride(0), _native.ptr(lens), blob.data_ptr(), g.data_ptr(),
                                  grad.data_ptr(), ld_grad, _native.ptr(raw), scratch.data_ptr(), npass, stream)
    assert rc == _native.FSEM_OK, rc
    assert bool((grad[:, L:] == 7.0).all())   # (columns at or past `length` are not written)
    return (grad[:, :L], raw) if want_raw else grad[:, :L]


def forward_entry(m, entry, rows, cols):
    lib = _native.load_dnsmos()
    B, L = rows.shape
    out = torch.empty(B * lib.fsem_dnsmos_segments(L), *cols, device=rows.device)
    ws = _native.workspace(lib.fsem_dnsmos_workspace_bytes(B, L), rows.device)
    rc = getattr(lib, entry)(rows.data_ptr(), B, L, rows.stride(0), None, m.blob(rows.device).data_ptr(), out.data_ptr(),
                             ws.data_ptr(), ws.numel(), _native.stream_handle(rows.device))
    assert rc == _native.FSEM_OK, rc
    return out


# ------------------------------------------------------------------ the forward
def test_scores_and_raw_outputs_are_the_forward_s(metric):
    x = dc.fixture("dnsmos_short").rows
    scores, _ = engine(metric, x)
    assert_bitwise(scores, metric.scores(x.cuda()), "differentiable_scores against scores")
    long = dc.fixture("dnsmos_long").rows[:, :160160].cuda().contiguous()   # two segments
    _, raw = c_entry(metric, long, [1.0, 1.0, 1.0], npass=1, want_raw=True)
    assert_bitwise(raw, forward_entry(metric, "fsem_dnsmos_raw_f32", long, (3,)), "the recomputed raw outputs")


# ------------------------------------------------------------------ against float64
@pytest.mark.parametrize("b", [0, 1, 2])
def test_gradient_against_float64(metric, b):
    row = dc.fixture("dnsmos_16k").rows[b:b + 1]
    keys = (0, 1, 2) if b == 0 else (2,)   # OVRL on every row, SIG and BAK on one
    _, want = gc.reference("dnsmos_16k", b, keys)
    worst = 0.0
    for j, k in enumerate(keys):
        g = [float(i == k) for i in range(3)]
        _, grad = engine(metric, row, g)
        err = gc.deviation(grad[0].cpu().numpy(), want[j])
        print(f"row {b} {DNSMOS.KEYS[k]}: deviation {err:.3e} (bar {BAR:.3e}), max |g| {np.abs(want[j]).max():.3e}")
        worst = max(worst, err)
    if b == 0:
        _, grad = engine(metric, row, gc.MIXED)
        err = gc.deviation(grad[0].cpu().numpy(), np.tensordot(np.asarray(gc.MIXED), want, 1))
        print(f"row {b} upstream {gc.MIXED}: deviation {err:.3e} (bar {BAR:.3e})")
        worst = max(worst, err)
    print(f"row {b}: worst deviation {worst:.3e} (bar {BAR:.3e})")
    assert worst <= BAR


def test_image_gradient_stage(metric):
    row = dc.fixture("dnsmos_16k").rows[:1].cuda()
    image = forward_entry(metric, "fsem_dnsmos_features_f32", row, (900, 161))
    got = c_entry(metric, row, [0.0, 0.0, 1.0], image=True)
    want = gc.image_gradients(image[0].cpu(), keys=(2,))[0]   # float64, on the engine's own image
    err = gc.deviation(got[0].cpu().numpy(), want)
    print(f"image gradient (OVRL): deviation {err:.3e} (bar {BAR_IMAGE:.3e}), max |g| {np.abs(want).max():.3e}")
    assert bool(torch.isfinite(got).all()) and err <= BAR_IMAGE


# ------------------------------------------------------------------ geometry
def test_two_overlapping_segments(metric):
    row = dc.fixture("dnsmos_long").rows[:, :160160]
    _, want = gc.gradients(row[0], keys=(2,))
    _, grad = engine(metric, row)
    err = gc.deviation(grad[0].cpu().numpy(), want[0])
    print(f"160160 samples, two segments: deviation {err:.3e} (bar {BAR:.3e})")
    assert err <= BAR


def test_a_short_row_collects_every_wrap(metric):
    row = dc.fixture("dnsmos_short").rows[0:1]   # 40000 samples: a sample feeds three or four segment positions
    _, want = gc.gradients(row[0], keys=(2,))
    _, grad = engine(metric, row)
    err = gc.deviation(grad[0].cpu().numpy(), want[0])
    print(f"40000 samples, wrapped: deviation {err:.3e} (bar {BAR:.3e})")
    assert err <= BAR


def test_a_ragged_batch(metric):
    src = dc.fixture("dnsmos_short").rows[[0, 2, 0]]
    lens = [40000, ONE_SEGMENT, 20000]
    pad = torch.zeros(3, 40010)
    for b, n in enumerate(lens):
        pad[b, :n] = src[b, :n]
    scores, grad = engine(metric, pad, lengths=lens)
    planted = pad.clone()
    for b, n in enumerate(lens):
        planted[b, n:] = float("nan")
    scores_p, grad_p = engine(metric, planted, lengths=lens)
    assert_bitwise((scores_p, grad_p), (scores, grad), "NaN planted past the lengths")
    for b, n in enumerate(lens):
        assert bool((grad[b, n:] == 0).all()) and bool(grad[b, :n].abs().max() > 0)
        _, alone = engine(metric, src[b:b + 1, :n].contiguous())
        assert_bitwise(grad[b:b + 1, :n], alone, f"row {b} ({n} samples) alone and unpadded")


# ------------------------------------------------------------------ one order for every sum
def test_reproducible_and_independent_of_position_ld_and_pass(metric):
    src = dc.fixture("dnsmos_short").rows
    x = short_rows()
    g = torch.tensor([[1.0, 0.0, 0.5], [0.0, 2.0, 0.0], [0.5, -1.0, 2.0]])
    _, grad = engine(metric, x, g)
    _, again = engine(metric, x, g)
    assert_bitwise(again, grad, "a second call")
    # row 0 alone against the same row last in a batch of three with another ld
    wide = torch.full((3, ONE_SEGMENT + 7), 3.0, device="cuda")
    wide[:, :ONE_SEGMENT] = x[[2, 1, 0]].cuda()
    moved = c_entry(metric, wide[:, :ONE_SEGMENT], g[[2, 1, 0]], ld_grad=ONE_SEGMENT + 3)
    assert_bitwise(moved[2:3], grad[0:1], "row 0 at position 2, ld 2507")
    assert_bitwise(c_entry(metric, x[0:1].cuda(), g[0:1]), grad[0:1], "row 0 alone")
    # pass sizes: a pass boundary inside a row's segments (2 + 2 + 1 segments)
    long = dc.fixture("dnsmos_long").rows[0]
    rows = torch.zeros(3, 160160)
    rows[0], rows[1], rows[2, :40000] = long[:160160], long[10000:170160], src[0]
    lens = [160160, 160160, 40000]
    base = c_entry(metric, rows.cuda(), g, lengths=lens, npass=16)
    for npass in (1, 3):
        assert_bitwise(c_entry(metric, rows.cuda(), g, lengths=lens, npass=npass), base, f"pass = {npass} against 16")
    assert bool((base[2, 40000:] == 0).all()) and bool(torch.isfinite(base).all())


def test_a_nonfinite_row(metric):
    x = short_rows()
    scores, grad = engine(metric, x)
    bad = x.clone()
    bad[1, 1234] = float("nan")
    scores_b, grad_b = engine(metric, bad)
    assert bool(torch.isnan(scores_b[1]).all()) and bool((grad_b[1] == 0).all())
    assert_bitwise((scores_b[[0, 2]], grad_b[[0, 2]]), (scores[[0, 2]], grad[[0, 2]]), "the rows beside it")
    # through the C entry with a seed on the flagged row as well, and a zero seed on another row
    got = c_entry(metric, bad.cuda(), [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    assert bool((got[1] == 0).all()) and bool((got[2] == 0).all())
    assert_bitwise(got[0:1], grad[0:1], "the row beside a flagged row and a zero seed")


# ------------------------------------------------------------------ another rate
def test_rows_at_8_khz():
    fx = dc.fixture("dnsmos_8k")
    m = DNSMOS(8000, use_gpu=True, weights=dc.WEIGHTS)
    scores, grad = engine(m, fx.rows, sr=8000)
    assert_bitwise(scores, m.scores(fx.rows.cuda(), 8000), "8 kHz: differentiable_scores against scores")
    est = fx.rows.double().requires_grad_(True)
    cpu = DNSMOS(8000, weights=dc.WEIGHTS).differentiable_scores(est, 8000)
    cpu[0, 2].backward()
    err = gc.deviation(grad[0].cpu().numpy(), est.grad[0].numpy())
    print(f"8 kHz row: deviation from CPU mode's float64 gradient {err:.3e} (bar {BAR:.3e})")
    assert err <= BAR


# ------------------------------------------------------------------ loss
def test_loss(metric):
    x = short_rows()
    scores, grad = engine(metric, x)
    bad = x.clone()
    bad[1, 7] = float("inf")
    est = bad.cuda().requires_grad_(True)
    loss = metric.loss(est)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    want = -float(scores[[0, 2], 2].double().mean())
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want)
    loss.backward()
    assert bool((est.grad[1] == 0).all()) and bool(torch.isfinite(est.grad).all())
    assert gc.deviation(est.grad[[0, 2]].cpu().numpy(), -grad[[0, 2]].double().cpu().numpy() / 2) <= 1e-6
    est = x.cuda().requires_grad_(True)
    metric.loss(est, key="SIG").backward()
    _, sig = engine(metric, x, [-1.0 / 3.0, 0.0, 0.0])   # (the mean's own upstream: another seed scale than 1 / 2 above)
    assert_bitwise(est.grad, sig, "loss(key='SIG') against the same upstream")
    allbad = torch.full_like(x, float("nan")).cuda().requires_grad_(True)
    loss = metric.loss(allbad)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert allbad.grad.shape == x.shape and bool((allbad.grad == 0).all())
    with pytest.raises(ValueError, match="key"):
        metric.loss(x.cuda(), key="MOS")
