"""STOI with gradients on the HIP engine (csrc/stoi_grad.hip) against the float64 reference of
tests/stoi_grad_cases.py: the forward bitwise against ``STOI.scores``, the gradient at every rate path (10 kHz
direct, 16 kHz, 8 and 48 kHz generic) for the incoming gradients (1, 0), (0, 1) and a random pair, also on rows
with a frame pair 20 peak exponents apart (the level equalisation the backward shares with the forward), the
conventions (rows without a gradient, zero envelopes, ragged rows), reproducibility, row layouts, a few
optimiser steps and one direct call of the C entries.

The gradient's bar is ``gc.bar()``: 32 x the largest error of the float32 torch restatement against the same
reference over the whole case set (measured 7.6e-6 ... 8.7e-6, a bar of 2.5e-4 ... 2.8e-4; the engine's own
worst row measured 1.5e-5).  The error of a row is max|g - g_ref| / max|g_ref|."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import STOI, _native

from . import stoi_grad_cases as gc
from .contract import bits

pytestmark = pytest.mark.gpu
NAMES = [s[0] for s in gc.SETS] + [gc.LONG[0], "zero", "odd"]
LR = 3e-4   # Adam's step, 0.3 ... 0.6 % of the rows' RMS: on the float64 CPU path ESTOI rises by 0.09 ... 0.23 per row


def engine(c, n, sr, lengths=None, g=None):
    """(stoi, estoi, grad) of host rows on the engine; grad for incoming g = (g_s, g_e) [B], or None."""
    m = STOI(sr, use_gpu=True)
    est = n.cuda().requires_grad_(True)
    s, e = m.differentiable_scores(c.cuda(), est, sr, lengths=lengths)
    assert s.is_cuda and s.dtype == e.dtype == torch.float32 and s.shape == e.shape == (c.shape[0],)
    if g is None:
        return s.detach(), e.detach(), None
    # (a NaN score times a zero incoming gradient would be NaN in the sum only: the rows' gradients come
    # from the incoming gradients alone)
    torch.autograd.backward([s, e], [g[0].cuda(), g[1].cuda()])
    assert est.grad.shape == n.shape and est.grad.dtype == torch.float32
    return s.detach(), e.detach(), est.grad


@functools.lru_cache(maxsize=None)
def engine_set(name, upstream):
    c, n, sr = gc.rows(name)
    B = c.shape[0]
    g = gc.incoming(B) if upstream == "random" else (torch.full((B,), upstream[0]), torch.full((B,), upstream[1]))
    return engine(c, n, sr, g=g) + (g,)


@pytest.mark.parametrize("name", NAMES)
def test_forward_is_scores_bitwise(name):
    c, n, sr = gc.rows(name)
    s, e, _, _ = engine_set(name, "random")
    s0, e0 = STOI(sr, use_gpu=True).scores(c.cuda(), n.cuda(), sr)
    assert s0.grad_fn is None and not s0.requires_grad
    np.testing.assert_array_equal(bits(s), bits(s0))
    np.testing.assert_array_equal(bits(e), bits(e0))
    want = gc.expected(name)["scores"]
    np.testing.assert_allclose(torch.stack([s, e], 1).cpu().numpy(), want, rtol=0, atol=3e-6, equal_nan=True)


@pytest.mark.parametrize("upstream", [(1.0, 0.0), (0.0, 1.0), "random"], ids=["stoi", "estoi", "random"])
@pytest.mark.parametrize("name", NAMES + ["gap"])   # "gap": a frame pair that the backward has to level-equalise
def test_gradient_against_the_reference(name, upstream):
    want = gc.expected(name)
    s, e, grad, g = engine_set(name, upstream)
    grad = grad.cpu().numpy()
    err = gc.row_errors(grad, gc.combine(want, g[0].numpy(), g[1].numpy()))
    print(f"{name} {upstream}: row errors {err}, bar {gc.bar():.3e}")
    assert np.isfinite(grad).all() and err.max() <= gc.bar()
    for b, seg in enumerate(gc.segments(name)):   # a row without a segment: NaN scores, exact zeros
        if seg == 0:
            assert np.isnan(float(s[b])) and (grad[b] == 0).all()
        else:
            assert np.abs(grad[b]).max() > 0 or name == "zero"
    if name == "zero":   # the all-zero estimate: score 0, a zero, finite gradient
        assert float(s[1]) == 0 and float(e[1]) == 0 and (grad[1] == 0).all() and np.abs(grad[0]).max() > 0


def test_a_non_finite_sample_zeroes_its_row_only():
    c, n, sr = gc.rows("16k")
    _, _, base, g = engine_set("16k", "random")
    bad = n.clone()
    bad[1, 5000] = float("nan")
    _, _, grad = engine(c, bad, sr, g=g)
    assert (grad[1] == 0).all()
    np.testing.assert_array_equal(bits(grad[[0, 2, 3]]), bits(base[[0, 2, 3]]))
    bad[1, 5000] = float("inf")
    assert (engine(c, bad, sr, g=g)[2][1] == 0).all()


def test_ragged_rows():
    c, n, sr = gc.rows("16k")
    lens = gc.RAGGED_LENGTHS
    want = gc.expected("16k", tuple(lens))
    g = gc.incoming(4)
    s, e, grad, = engine(c, n, sr, lengths=lens, g=g)
    err = gc.row_errors(grad.cpu().numpy(), gc.combine(want, g[0].numpy(), g[1].numpy()))
    assert err.max() <= gc.bar()
    for b, nb in enumerate(lens):
        assert (grad[b, nb:] == 0).all()
        # the unpadded row scored alone
        s1, e1, g1 = engine(c[b:b + 1, :nb], n[b:b + 1, :nb], sr, g=(g[0][b:b + 1], g[1][b:b + 1]))
        np.testing.assert_array_equal(bits(s1), bits(s[b:b + 1]))
        scale = float(g1.abs().max())
        assert float((g1[0] - grad[b, :nb]).abs().max()) <= gc.bar() * scale
    assert torch.isnan(s[3]) and (grad[3] == 0).all() and float(grad[1].abs().max()) > 0
    # the padding is never looked at
    c2, n2 = c.clone(), n.clone()
    c2[1, lens[1]:], n2[1, lens[1]:] = float("nan"), float("inf")
    np.testing.assert_array_equal(bits(engine(c2, n2, sr, lengths=lens, g=g)[2]), bits(grad))


def test_reproducible_and_batch_independent():
    c, n, sr = gc.rows("16k")
    _, _, base, g = engine_set("16k", "random")
    np.testing.assert_array_equal(bits(engine(c, n, sr, g=g)[2]), bits(base))
    for b in (1, 3):
        alone = engine(c[b:b + 1], n[b:b + 1], sr, g=(g[0][b:b + 1], g[1][b:b + 1]))[2]
        np.testing.assert_array_equal(bits(alone[0]), bits(base[b]))
    # the long row alone and as row 1 of a batch of two (other segment waves, other workgroups)
    c, n, sr = gc.rows(gc.LONG[0])
    _, _, base, g = engine_set(gc.LONG[0], "random")
    two = engine(torch.cat([c, c]), torch.cat([n * 0.5, n]), sr, g=(g[0].repeat(2), g[1].repeat(2)))[2]
    np.testing.assert_array_equal(bits(two[1]), bits(base[0]))


def test_row_layouts():
    c, n, sr = gc.rows("16k")
    _, _, base, g = engine_set("16k", "random")
    m = STOI(sr, use_gpu=True)
    wide, cwide = torch.zeros(4, 16000 + 36).cuda(), torch.zeros(4, 16000 + 36).cuda()
    wide[:, 12:16012], cwide[:, 12:16012] = n.cuda(), c.cuda()
    est = wide.requires_grad_(True)
    s, e = m.differentiable_scores(cwide[:, 12:16012], est[:, 12:16012], sr)   # slices: the engine reads them in place
    torch.autograd.backward([s, e], [g[0].cuda(), g[1].cuda()])
    np.testing.assert_array_equal(bits(est.grad[:, 12:16012]), bits(base))
    assert (est.grad[:, :12] == 0).all() and (est.grad[:, 16012:] == 0).all()
    # an odd length against its zero-padded copy with lengths
    c, n, sr = gc.rows("odd")
    _, _, odd, g = engine_set("odd", "random")
    pad = torch.nn.functional.pad
    padded = engine(pad(c, (0, 3)), pad(n, (0, 3)), sr, lengths=[gc.ODD_LENGTH] * 4, g=g)[2]
    np.testing.assert_array_equal(bits(padded[:, :gc.ODD_LENGTH]), bits(odd))
    # half precision estimates: cast to float32, the gradient back in their dtype
    half = n.cuda().to(torch.bfloat16).requires_grad_(True)
    m.loss(c.cuda(), half, sr).backward()
    assert half.grad.dtype == torch.bfloat16 and bool(torch.isfinite(half.grad.float()).all())


def test_loss_and_refusals():
    c, n, sr = gc.rows("10k")
    m = STOI(10000, use_gpu=True)
    est = n.cuda().requires_grad_(True)
    want = gc.expected("10k")
    for key, col in (("STOI", 0), ("ESTOI", 1)):
        est.grad = None
        loss = m.loss(c.cuda(), est, key=key)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert abs(float(loss.detach()) + np.nanmean(want["scores"][:, col])) <= 3e-6
        loss.backward()
        err = gc.row_errors(est.grad.cpu().numpy(), -want["gs" if col == 0 else "ge"] / 3)
        assert err.max() <= gc.bar() and (est.grad[2] == 0).all()
    short = n[:, :3000].cuda().requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="Not enough non-silent frames"):
        loss = m.loss(c[:, :3000].cuda(), short)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert (short.grad == 0).all()
    with pytest.raises(NotImplementedError, match="constants"):
        m.loss(c.cuda().requires_grad_(True), est)
    fan = STOI(10000, use_gpu=True)
    fan._fanout = object()   # (stands in for a metric built with devices=)
    with pytest.raises(NotImplementedError, match="devices"):
        fan.loss(c.cuda(), est)


def test_it_trains():
    c, n, sr = gc.rows("16k")
    m = STOI(sr, use_gpu=True)
    cd = c.cuda()
    est = n.cuda().clone().requires_grad_(True)
    opt = torch.optim.Adam([est], lr=LR)
    before = m.scores(cd, est.detach(), sr)[1]
    for _ in range(5):
        opt.zero_grad()
        m.loss(cd, est, sr, key="ESTOI").backward()
        opt.step()
    after = m.scores(cd, est.detach(), sr)[1]
    print("ESTOI before", before.tolist(), "after", after.tolist())
    assert bool((after > before).all())


def test_c_entries_directly():
    lib = _native.load()
    c, n, sr = gc.rows("8k")
    B, L = c.shape
    ld, grad_ld = L + 8, L + 12
    pad = torch.nn.functional.pad
    cd, nd = pad(c, (0, 8)).cuda(), pad(n, (0, 8)).cuda()
    s = torch.empty(B, device="cuda")
    e = torch.empty(B, device="cuda")
    seg = torch.empty(B, dtype=torch.int32, device="cuda")
    nfl = lib.fsem_stoi_state_floats(B, L, sr)
    state = torch.empty(nfl, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _native.stream_handle(cd.device)
    assert lib.fsem_stoi_state_f32(p(cd), p(nd), B, L, ld, None, sr, p(s), p(e), p(seg), p(state), st) == _native.FSEM_OK
    assert seg.tolist() == gc.segments("8k")
    s0, e0, base, g = engine_set("8k", "random")
    np.testing.assert_array_equal(bits(s), bits(s0))
    np.testing.assert_array_equal(bits(e), bits(e0))
    grad = torch.full((B, grad_ld), 7.0, device="cuda")
    gs, ge = g[0].cuda(), g[1].cuda()
    for _ in range(2):   # (the state may be read again)
        assert lib.fsem_stoi_grad_f32(p(nd), B, L, ld, None, sr, p(state), p(gs), p(ge), p(grad), grad_ld, st) == \
            _native.FSEM_OK
        np.testing.assert_array_equal(bits(grad[:, :L]), bits(base))
        assert (grad[:, L:] == 7.0).all()   # the padding columns are not written
