"""SRMR with gradients on the HIP engine (csrc/srmr_grad.hip) against the float64 statement of
tests/srmr_grad_cases.py: the forward bitwise ``scores()``, the gradient under a bar computed from the statement
alone, the exact zeros, reproducibility and independence of the batch and of the scratch's row passes, the
row's scale, the grid limit, a short ascent, and row layouts and streams."""
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SRMR, _native

from . import contract
from . import srmr_cases as sc
from . import srmr_grad_cases as gc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def metric(sr: int) -> SRMR:
    return SRMR(sr, use_gpu=True)


def engine(rows, sr, lens=None, g=None):
    """(scores [B] float32, gradient [B, L] float32, both on the device) for the incoming gradient g (ones)."""
    est = rows.cuda().requires_grad_(True)
    s = metric(sr).differentiable_scores(est, lengths=None if lens is None else list(lens))
    assert s.is_cuda and s.dtype == torch.float32 and s.shape == (rows.shape[0],)
    s.backward((torch.ones(rows.shape[0]) if g is None else g).to(s))
    assert est.grad.dtype == torch.float32 and est.grad.shape == rows.shape
    return s.detach(), est.grad


def pass_rows(length: int) -> int:
    return int(_native.load().fsem_srmrgrad_pass_rows(length))


def row_of(kind, seed, sr, n) -> torch.Tensor:
    return torch.from_numpy(np.array(sc.reference(kind, seed, sr, n)[0]))[None]


@pytest.mark.parametrize("name", sorted(gc.SETS))
@pytest.mark.parametrize("sr", gc.RATES)
def test_forward_is_scores_and_gradient_is_under_the_bar(sr, name):
    specs = gc.SETS[name](sr)
    rows, lens = gc.batch_of(specs)   # one ragged batch, NaN / 1e30 past each length
    want = gc.expected_batch(specs)
    bar = gc.engine_bar(specs)
    s, grad = engine(rows, sr, lens)
    contract.assert_bitwise(s, metric(sr).scores(rows.cuda(), lengths=lens), f"{sr} {name}: forward")
    err = gc.row_errors(grad.cpu().numpy(), want)
    g = gc.incoming(len(lens))
    err_g = gc.row_errors(engine(rows, sr, lens, g)[1].cpu().numpy(), want * g.double().numpy()[:, None])
    yard = gc.row_errors(gc.expected_batch(specs, True), want)
    print(f"gpu {sr} {name}: row errors {' '.join(f'{v:.2e}' for v in err)} (ones), "
          f"{' '.join(f'{v:.2e}' for v in err_g)} (random incoming); bar {bar:.2e}; the complex64 statement "
          f"{' '.join(f'{v:.2e}' for v in yard)}")
    assert bool(torch.isfinite(grad).all())
    assert err.max() <= bar and err_g.max() <= bar
    for b, k in enumerate(lens):
        assert bool((grad[b, k:] == 0).all())
        assert bool((grad[b, max(gc.nend_of(k, sr) - 1, 0):] == 0).all())


@pytest.mark.parametrize("sr", gc.RATES)
def test_exact_zeros(sr):
    wi, wl = sc.geometry(sr)
    x = row_of("noisy", 3, sr, 2 * sr)[0]
    n = 2 * sc.TILE + wi + 77
    rows = torch.stack([x[:n], x[:n], x[:n], torch.zeros(n), x[sr // 2:sr // 2 + n], x[:n], x[:n]])
    rows[1, 100] = float("nan")
    rows[5, n - 1] = float("inf")
    lens = [n, n, wl - 1, n, wl + wi + 5, n, n]
    g = torch.tensor([1.0, 1.0, 1.0, 1.0, -0.5, 1.0, 0.0])
    s, grad = engine(rows, sr, lens, g)
    contract.assert_bitwise(s, metric(sr).scores(rows.cuda(), lengths=lens), f"{sr}: forward")
    assert bool(torch.isfinite(s[[0, 4, 6]]).all()) and bool(torch.isnan(s[[1, 2, 3, 5]]).all())
    # a NaN sample, no frame, digitally silent, an infinite sample, a zero incoming gradient
    assert bool((grad[[1, 2, 3, 5, 6]] == 0).all())
    for b in (0, 4):
        nend = gc.nend_of(lens[b], sr)
        assert bool((grad[b, nend - 1:] == 0).all()) and float(grad[b, :nend - 1].abs().max()) > 0
    # the rows beside them are the rows alone
    for b in (0, 4):
        _, alone = engine(rows[b:b + 1, :lens[b]], sr, g=g[b:b + 1])
        contract.assert_bitwise(alone, grad[b:b + 1, :lens[b]], f"{sr}: row {b} alone")
    # the loss: -mean over the scored rows; no scored row: a zero with a zero gradient
    est = rows.cuda().requires_grad_(True)
    loss = metric(sr).loss(est, lengths=lens)
    want = -float(s[[0, 4, 6]].double().mean())
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want)
    loss.backward()
    assert bool((est.grad[[1, 2, 3, 5]] == 0).all()) and bool(torch.isfinite(est.grad).all())
    est = rows[1:4].cuda().requires_grad_(True)
    loss = metric(sr).loss(est, lengths=lens[1:4])
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert est.grad.shape == (3, n) and bool((est.grad == 0).all())
    # rows of no samples: the scores, and an empty gradient
    est = rows[:, :0].cuda().requires_grad_(True)
    s0 = metric(sr).differentiable_scores(est)
    assert s0.shape == (7,) and bool(torch.isnan(s0).all())
    s0.sum().backward()
    assert est.grad.shape == (7, 0)
    fan = SRMR(sr, use_gpu=True)
    fan._fanout = object()   # (stands in for a metric built with devices=)
    with pytest.raises(NotImplementedError, match="devices= is not supported with gradients"):
        fan.loss(rows.cuda())


@pytest.mark.parametrize("sr", gc.RATES)
def test_reproducible_and_independent_of_the_batch_and_the_pass(sr):
    specs = gc.edge_specs(sr)
    rows, lens = gc.batch_of(specs)
    B, L = rows.shape
    g = gc.incoming(B)
    s, grad = engine(rows, sr, lens, g)
    contract.assert_bitwise(engine(rows, sr, lens, g), (s, grad), f"{sr}: a second run")
    for b, k in enumerate(lens):
        _, alone = engine(rows[b:b + 1, :k], sr, g=g[b:b + 1])
        contract.assert_bitwise(alone, grad[b:b + 1, :k], f"{sr}: row {b} (n = {k}) alone and unpadded")
    # a batch that spans two row passes of the scratch: the rows on both sides of the border
    P = pass_rows(L)
    reps = -(-(P + B) // B)
    assert 0 < P < reps * B
    _, big = engine(rows.repeat(reps, 1), sr, lens * reps, g.repeat(reps))
    for b in sorted({0, P - 1, P, P + 1, reps * B - 1}):
        contract.assert_bitwise(big[b:b + 1], grad[b % B:b % B + 1], f"{sr}: row {b} of {reps * B}, pass of {P}")


@pytest.mark.parametrize("sr", gc.RATES)
def test_scale(sr):
    spec = ("reverberated", 1, sr, sr)
    x = row_of(*spec)
    want = gc.expected(*spec)[1][None]
    bar = gc.engine_bar(gc.parity_specs(sr))
    _, base = engine(x, sr)
    top = float(np.abs(want).max())
    for gain in (1e-3, 1.0, 1e3):
        _, grad = engine(x * gain, sr)
        diff = float((gain * grad.double() - base.double()).abs().max()) / top
        print(f"gpu {sr}: gain {gain:g}: max|gain grad(gain x) - grad(x)| / max|g_ref| = {diff:.2e}; bar {bar:.2e}")
        assert diff <= bar
    dot = abs(float((base[0].double().cpu() * x[0].double()).sum()))
    dot_ref = abs(float((torch.from_numpy(want[0].copy()) * x[0].double()).sum()))
    print(f"gpu {sr}: |sum g x| = {dot:.3e}, the statement's {dot_ref:.3e}")
    assert dot <= dot_ref + bar * top * float(x.double().abs().sum())


def test_past_the_grid_limit():
    sr, n, NB = 8000, 2048, 65536
    x = row_of("harmonic", 1, sr, n)   # one frame
    P = pass_rows(n)
    _, alone = engine(x, sr)
    assert float(alone.abs().max()) > 0
    _, big = engine(x.cuda().expand(NB, n).contiguous(), sr)
    for b in sorted({0, P - 1, P, 65534, 65535}):
        contract.assert_bitwise(big[b:b + 1], alone, f"row {b} of {NB}, passes of {P}")


@pytest.mark.parametrize("sr", gc.RATES)
def test_ascent(sr):
    """The trace of tests/test_srmr_grad_cpu.py::test_ascent holds on the engine: every step raises scores()."""
    first, trace = gc.ascent(metric(sr), "cuda")
    print(f"gpu {sr}: SRMR {first:.4f} -> {' '.join(f'{v:.4f}' for v in trace)}")
    assert all(b > a for a, b in zip([first] + trace, trace))


def test_streams_and_layouts():
    sr = 16000
    specs = gc.parity_specs(sr)[:2]
    rows, lens = gc.batch_of(specs, fill=False)
    B, L = rows.shape
    g = gc.incoming(B)
    s, grad = engine(rows, sr, lens, g)
    contract.assert_bitwise(contract.on_side_stream(lambda: engine(rows, sr, lens, g)), (s, grad), "a side stream")
    # a view of a wider tensor at a 3-float offset with an odd row stride (ld > length)
    wide = torch.full((B, L + 13), 7.0).cuda()
    wide[:, 3:3 + L] = rows.cuda()
    est = wide.requires_grad_(True)
    got = metric(sr).differentiable_scores(est[:, 3:3 + L], lengths=lens)
    got.backward(g.to(got))
    contract.assert_bitwise((got.detach(), est.grad[:, 3:3 + L]), (s, grad), "a strided view")
    assert bool((est.grad[:, :3] == 0).all()) and bool((est.grad[:, 3 + L:] == 0).all())
    # the C entry on that view: nothing past `length` is written, the scratch reused
    lib = _native.load()
    view = wide.detach()[:, 3:3 + L]
    ld = view.stride(0)
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    _, energies = metric(sr).scores(view, lengths=lens, return_energies=True)
    scratch = torch.empty(lib.fsem_srmrgrad_scratch_bytes(B, L), dtype=torch.uint8, device="cuda")
    gd = g.cuda()
    for _ in range(2):
        out = torch.full((B, ld), 5.0, device="cuda")
        rc = lib.fsem_srmrgrad_f32(view.data_ptr(), B, L, ld, lens_d.data_ptr(), sr, energies.data_ptr(), gd.data_ptr(),
                                   scratch.data_ptr(), out.data_ptr(), _native.stream_handle(out.device))
        assert rc == 0
        contract.assert_bitwise(out[:, :L], grad, "the C entry")
        assert bool((out[:, L:] == 5.0).all())
    assert lib.fsem_srmrgrad_scratch_bytes(0, L) == 0 and lib.fsem_srmrgrad_scratch_bytes(B, 0) == 0
    assert lib.fsem_srmrgrad_f32(view.data_ptr(), B, L, ld, None, 22050, energies.data_ptr(), gd.data_ptr(),
                                 scratch.data_ptr(), out.data_ptr(), None) == _native.FSEM_ERATE
