"""LSD with gradients without a GPU: the five C entries (declared, exported, bound; the state query; every
refusal answered on the host before any launch), the float64 statement of tests/lsd_grad_cases.py against
central differences of ``lsd_cases.expected_row``, CPU mode (``_cpu.lsd64`` in float64 under torch's autograd)
against the statement in scores and gradients on every parity case, the conventions, and ``loss``."""
import ctypes

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import LSD, _build, _native

from . import contract
from . import lsd_cases as lc
from . import lsd_grad_cases as gc

ENTRIES = ("fsem_lsd_grad_state_floats", "fsem_lsd_grad_f32", "fsem_lsd_grad_rate_state_floats",
           "fsem_lsd_grad_rate_f32")


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


def test_entries_are_declared_exported_and_bound(lib):
    contract.entries_are_declared_exported_and_bound(lib, "fsem_lsd_", ENTRIES)   # (the forward's: libfsem_lsd.so)
    old = {"fsem_resample_length", "fsem_resample_f32", "fsem_resample_rows_f32"}
    contract.entries_are_declared_exported_and_bound(lib, "fsem_resample_", ("fsem_resample_rows_grad_f32",), old)
    assert "lsd_grad.hip" in _build.SOURCES and "fsem_lsd_kernels.h" in _build.HEADERS
    assert "lsd_grad.hip" not in _build.library("lsd").sources
    assert not any(n.startswith("fsem_lsd_grad") or "grad" in n for n in _native.LSD_SIGNATURES)


def test_state_floats(lib):
    prev = 0
    for L in (1, 255, 256, 4096, 16000, 160000):
        n1, n4 = lib.fsem_lsd_grad_state_floats(1, L), lib.fsem_lsd_grad_state_floats(4, L)
        assert 0 < n1 <= n4 and n1 >= prev, L
        assert 4 * n1 >= 8 * L   # ybar in double
        prev = n1
    assert lib.fsem_lsd_grad_state_floats(5, 16000) >= lib.fsem_lsd_grad_state_floats(4, 16000)
    assert lib.fsem_lsd_grad_state_floats(1, 1 << 29) > 0
    for B, L in ((0, 16000), (-1, 16000), (4, 0), (4, -1), (4, (1 << 29) + 1)):
        assert lib.fsem_lsd_grad_state_floats(B, L) == 0, (B, L)
        assert lib.fsem_lsd_grad_rate_state_floats(B, L, 8000) == 0, (B, L)
    # other rates: the 16 kHz state at the resampled length and both rows in double
    assert lib.fsem_lsd_grad_rate_state_floats(4, 16000, 16000) == lib.fsem_lsd_grad_state_floats(4, 16000)
    for sr, L in ((8000, 8000), (48000, 48000)):
        n = lib.fsem_lsd_grad_rate_state_floats(4, L, sr)
        assert n >= lib.fsem_lsd_grad_state_floats(4, 16000) + 4 * 16000 * 4 > 0
        assert lib.fsem_lsd_grad_rate_state_floats(5, L, sr) >= n
    for B, L, sr in ((4, 16000, 0), (4, 16000, 44101), (4, 1 << 29, 8000)):   # no kernel; 2^30 resampled samples
        assert lib.fsem_lsd_grad_rate_state_floats(B, L, sr) == 0, (B, L, sr)


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(256), None
    big = (1 << 29) + 4
    EINVAL, ERATE, OK = _native.FSEM_EINVAL, _native.FSEM_ERATE, _native.FSEM_OK
    bwd = contract.by_name(lib.fsem_lsd_grad_f32, "ref deg batch length ld lengths g state grad grad_ld", null)
    ok = dict(ref=p, deg=p, batch=3, length=16000, ld=16000, lengths=null, g=p, state=p, grad=p, grad_ld=16000)
    contract.refusals(bwd, ok, contract.nulled(EINVAL, "ref deg g state grad") + contract.each(
        EINVAL, dict(batch=0), dict(batch=-1), dict(length=0), dict(length=-4), dict(ld=15999), dict(grad_ld=15999),
        dict(length=big, ld=big, grad_ld=big)))
    rate = contract.by_name(lib.fsem_lsd_grad_rate_f32, "ref deg batch length ld lengths sr g state grad grad_ld", null)
    contract.refusals(rate, dict(ok, sr=8000), contract.nulled(EINVAL, "ref deg g state grad") + contract.each(
        EINVAL, dict(batch=0), dict(batch=-1), dict(length=0), dict(ld=15999), dict(grad_ld=15999),
        dict(length=big, ld=big, grad_ld=big), dict(length=1 << 29, ld=1 << 29, grad_ld=1 << 29))
        + contract.each(ERATE, dict(sr=0), dict(sr=44101)))
    rsg = contract.by_name(lib.fsem_resample_rows_grad_f32, "g rows n_in ld_out lengths grad ld_in orig new", null)
    okr = dict(g=p, rows=3, n_in=8000, ld_out=16000, lengths=null, grad=p, ld_in=8000, orig=8000, new=16000)
    contract.refusals(rsg, okr, contract.nulled(EINVAL, "g grad") + contract.each(
        EINVAL, dict(rows=-1), dict(n_in=-1), dict(ld_in=7999), dict(ld_out=15999), dict(n_in=big, ld_in=big, ld_out=2 * big))
        + contract.each(ERATE, dict(new=8000), dict(orig=44100, new=16001), dict(orig=0))
        + contract.each(OK, dict(rows=0), dict(rows=0, lengths=p), dict(n_in=0, ld_in=0, ld_out=0)))


@pytest.mark.parametrize("n", [300, 700])
def test_statement_against_central_differences(n):
    c, y = lc.speech_rows(1, n, seed=31)
    s, h = c[0].double().numpy(), y[0].double().numpy()
    value, grad = gc.expected_row(s, h)
    assert abs(value - lc.expected_row(s, h)) <= 1e-12 * value
    rng = np.random.default_rng(n)
    scale = np.abs(grad).max()
    for i in rng.choice(n, 12, replace=False):
        quot = []
        for eps in (1e-6, 5e-7):   # (in the quotient's flat range: the two steps agree)
            d = np.zeros(n)
            d[i] = eps
            quot.append((lc.expected_row(s, h + d) - lc.expected_row(s, h - d)) / (2 * eps))
        print(f"n {n} coordinate {i}: gradient {grad[i]:.6e}, quotient - gradient {quot[0] - grad[i]:.2e} / "
              f"{quot[1] - grad[i]:.2e}")
        assert abs(quot[0] - grad[i]) <= 1e-6 * scale and abs(quot[1] - grad[i]) <= 1e-6 * scale


def cpu_mode(name, g=None):
    """(scores [B], gradient [B, L]) of CPU mode on a named case for the incoming gradient g (ones)."""
    c, n, sr, lens = gc.rows(name)
    est = n.double().requires_grad_(True)   # (a float64 leaf: the gradient arrives unrounded)
    lsd = LSD(sr).differentiable_scores(c, est, sr, lengths=None if lens is None else list(lens))
    assert lsd.dtype == torch.float64 and lsd.shape == (c.shape[0],)
    g = torch.ones(c.shape[0]) if g is None else g
    (lsd * g.double()).sum().backward()
    return lsd.detach().numpy(), est.grad.numpy()


@pytest.mark.parametrize("name", gc.PARITY)
def test_cpu_mode_against_the_statement(name):
    want_s, want_g = gc.expected(name)
    assert np.isfinite(want_s).all() and np.isfinite(want_g).all() and (np.abs(want_g).max(axis=1) > 0).all()
    scores, grad = cpu_mode(name)
    lc.assert_close(scores, want_s, f"cpu mode {name}")
    err = gc.row_errors(grad, want_g)
    print(f"cpu mode {name}: worst gradient error {err.max():.3e} of the row's largest; float32 autograd "
          f"{' '.join(f'{v:.1e}' for v in gc.float32_autograd(name))}")
    assert np.isfinite(grad).all() and err.max() <= gc.RTOL_CPU
    g = gc.incoming(len(want_s))
    _, grad = cpu_mode(name, g)
    assert gc.row_errors(grad, want_g * g.double().numpy()[:, None]).max() <= gc.RTOL_CPU
    lens = gc.rows(name)[3]
    if lens is not None:
        for b, k in enumerate(lens):
            assert (grad[b, k:] == 0).all()


def test_the_bars():
    assert gc.BAR == 4 * gc.MEASURED <= gc.BAR_LIMIT and gc.BAR_RESAMPLE == 4 * gc.MEASURED_RESAMPLE <= gc.BAR_LIMIT


def test_conventions_in_cpu_mode():
    m = LSD(16000)
    c, n, _, _ = gc.rows("speech")
    want_s, want_g = gc.expected("speech")
    # a non-finite sample, in either operand: NaN and a zero row, the other rows bitwise unchanged
    est = n.double().requires_grad_(True)
    good = m.differentiable_scores(c, est)
    good.sum().backward()
    for where in ("estimate", "clean"):
        cb, nb = c.clone(), n.clone()
        (nb if where == "estimate" else cb)[1, 5000] = float("nan") if where == "estimate" else float("inf")
        bad = nb.double().requires_grad_(True)
        lsd = m.differentiable_scores(cb, bad)
        assert bool(torch.isnan(lsd[1])) and bool(torch.isfinite(lsd[[0, 2, 3]]).all())
        lsd[[0, 2, 3]].sum().backward()
        assert (bad.grad[1] == 0).all()
        contract.assert_bitwise(bad.grad[[0, 2, 3]], est.grad[[0, 2, 3]], where)
        contract.assert_bitwise(lsd[[0, 2, 3]], good[[0, 2, 3]], where)
    # silent clean, silent estimate, both silent: exact zeros (rows 1 .. 3 of the edge rows), finite elsewhere
    ce, ne = lc.edge_rows()
    est = ne.double().requires_grad_(True)
    lsd = m.differentiable_scores(ce, est)
    lsd.sum().backward()
    assert bool(torch.isfinite(lsd).all()) and bool(torch.isfinite(est.grad).all())
    assert (est.grad[1:4] == 0).all()
    for b in (0, 4, 5):   # identical up to a gain: a residual of cancelling terms, finite
        w = gc.expected_row(ce[b].numpy(), ne[b].numpy())[1]
        print(f"{lc.EDGE_NAMES[b]}: max |g| {float(est.grad[b].abs().max()):.3e}, statement {np.abs(w).max():.3e}")
    # lengths: zeros past each length, each row as the row alone
    lens = [16000, 700, 255, 1]
    est = n.double().requires_grad_(True)
    lsd = m.differentiable_scores(c, est, lengths=lens)
    lsd.sum().backward()
    for b, k in enumerate(lens):
        s, g = gc.expected_row(c[b, :k].numpy(), n[b, :k].numpy())
        assert (est.grad[b, k:] == 0).all() and bool(torch.isfinite(est.grad[b]).all())
        assert abs(float(lsd[b].detach()) - s) <= lc.RTOL * s
        if k > 1:   # (one sample: a residual of two cancelling terms)
            assert gc.row_errors(est.grad[b:b + 1, :k].numpy(), g[None]).max() <= gc.RTOL_CPU
    # a batch of no samples, and no rows
    empty = n[:, :0].clone().requires_grad_(True)
    lsd = m.differentiable_scores(c[:, :0], empty)
    assert lsd.shape == (4,) and np.allclose(lsd.detach().numpy(), lc.LN1E8, rtol=1e-12)
    lsd.sum().backward()
    assert empty.grad.shape == (4, 0)
    assert m.differentiable_scores(c[:0], n[:0].clone().requires_grad_(True)).shape == (0,)


def test_loss():
    m = LSD(16000)
    c, n, _, _ = gc.rows("speech")
    want_s, want_g = gc.expected("speech")
    est = n.clone().requires_grad_(True)
    loss = m.loss(c, est)
    assert loss.dtype == torch.float64 and loss.dim() == 0
    assert abs(float(loss.detach()) - want_s.mean()) <= 1e-12 * want_s.mean()
    loss.backward()
    assert est.grad.dtype == torch.float32
    np.testing.assert_allclose(est.grad.numpy(), (want_g / 4).astype(np.float32), rtol=2.0 ** -22, atol=1e-12)
    # the mean is over the rows with a finite score
    bad = n.clone()
    bad[2, 100] = float("nan")
    est = bad.requires_grad_(True)
    loss = m.loss(c, est)
    assert abs(float(loss.detach()) - want_s[[0, 1, 3]].mean()) <= 1e-12 * want_s.mean()
    loss.backward()
    assert (est.grad[2] == 0).all()
    np.testing.assert_allclose(est.grad[[0, 1, 3]].numpy(), (want_g[[0, 1, 3]] / 3).astype(np.float32), rtol=2.0 ** -22,
                               atol=1e-12)
    # no finite row: a zero that carries a zero gradient
    allbad = torch.full_like(n, float("nan")).requires_grad_(True)
    loss = m.loss(c, allbad)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert allbad.grad.shape == n.shape and (allbad.grad == 0).all()
    # the refusals; half precision estimates get their gradient in their own dtype
    src = c.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="constants"):
        m.loss(src, n)
    with pytest.raises(NotImplementedError, match="constants"):
        m.differentiable_scores(src, n.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="sample_rate"):
        LSD(8000).loss(c, n)   # an 8 kHz metric must be told its rows' rate
    half = n.to(torch.bfloat16).requires_grad_(True)
    m.loss(c, half).backward()
    assert half.grad.dtype == torch.bfloat16 and bool(torch.isfinite(half.grad.float()).all())


def test_devices_are_refused():
    class Shards:   # (a fan-out needs GPUs to construct: stand in for one)
        pass

    m = LSD(16000)
    m._fanout = Shards()
    c, n, _, _ = gc.rows("speech")
    with pytest.raises(NotImplementedError, match="devices"):
        m.differentiable_scores(c, n)
    with pytest.raises(NotImplementedError, match="devices"):
        m.loss(c, n)
