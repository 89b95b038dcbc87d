"""SRMR with gradients without a GPU: the float64 statement of tests/srmr_grad_cases.py against central
differences of the forward statement, the package's CPU mode (``_cpu.srmr64``) against the statement, and the
host rules of ``SRMR.differentiable_scores`` / ``SRMR.loss``."""
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SRMR

from . import srmr_cases as sc
from . import srmr_grad_cases as gc


@functools.lru_cache(maxsize=None)
def metric(sr: int) -> SRMR:
    return SRMR(sr, use_gpu=False)


def cpu_mode(rows, sr, lens=None, g=None):
    """(scores [B] float64, gradient [B, L] in the rows' dtype) of CPU mode for the incoming gradient g (ones)."""
    est = rows.clone().requires_grad_(True)
    s = metric(sr).differentiable_scores(est, lengths=lens)
    assert s.dtype == torch.float64 and s.shape == (rows.shape[0],)
    s.backward(torch.ones_like(s) if g is None else g.to(s))
    assert est.grad.shape == rows.shape
    return s.detach(), est.grad


def same_or_nan(a, b) -> bool:
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("sr", gc.RATES)
def test_statement_against_central_differences(sr):
    assert gc.FD_BAR < gc.FD_LIMIT
    for spec in gc.parity_specs(sr):
        x = np.array(sc.reference(*spec)[0], dtype=np.float64)
        score, g = gc.expected(*spec)
        assert sc.rel(score, sc.reference(*spec)[1][0]) <= 1e-12   # the statement's forward is srmr_cases'
        d = np.random.default_rng(5).standard_normal(len(x))
        d /= np.linalg.norm(d)

        def f(v):
            return sc.score_of(sc.energies_of(sc.analytic_envelopes(v, sr), sr), sr)

        fd = (f(x + gc.FD_STEP * d) - f(x - gc.FD_STEP * d)) / (2 * gc.FD_STEP)
        rel = abs(float(g @ d) - fd) / abs(fd)
        print(f"{sr} {spec[0]}: central difference {fd:.9e}, statement {float(g @ d):.9e}, relative {rel:.2e}; "
              f"bar {gc.FD_BAR:.2e}")
        assert rel <= gc.FD_BAR
        nend = gc.nend_of(len(x), sr)
        assert (g[nend - 1:] == 0).all() and np.abs(g[:nend - 1]).max() > 0
        # SRMR does not depend on the row's scale
        assert abs(float(g @ x)) <= 1e-9 * np.abs(g).max() * np.abs(x).sum()


@pytest.mark.parametrize("name", sorted(gc.SETS))
@pytest.mark.parametrize("sr", gc.RATES)
def test_cpu_mode_against_the_statement(sr, name):
    specs = gc.SETS[name](sr)
    rows, lens = gc.batch_of(specs)
    want = gc.expected_batch(specs)
    rows = rows.double()   # both sides are float64
    for label, g in (("ones", torch.ones(len(lens))), ("random", gc.incoming(len(lens)))):
        s, grad = cpu_mode(rows, sr, lens, g)
        err = gc.row_errors(grad.numpy(), want * g.double().numpy()[:, None])
        print(f"cpu {sr} {name} ({label}): row errors {' '.join(f'{v:.2e}' for v in err)}; bar {gc.CPU_BAR:.2e}")
        assert grad.dtype == torch.float64 and bool(torch.isfinite(grad).all())
        assert err.max() <= gc.CPU_BAR
        for b, k in enumerate(lens):
            assert bool((grad[b, k:] == 0).all())
            assert bool((grad[b, max(gc.nend_of(k, sr) - 1, 0):] == 0).all())
    # the scores are scores()
    assert same_or_nan(s.float(), metric(sr).scores(rows.float(), lengths=lens))


@pytest.mark.parametrize("sr", gc.RATES)
def test_host_rules(sr):
    wi, wl = sc.geometry(sr)
    x = torch.from_numpy(np.array(sc.reference("noisy", 3, sr, 2 * sr)[0]))
    n = wl + 3 * wi + 77
    rows = torch.stack([x[:n], x[:n], x[:n], torch.zeros(n), x[sr:sr + n]])
    rows[1, 100] = float("nan")
    lens = [n, n, wl - 1, n, wl + wi + 5]
    s, grad = cpu_mode(rows, sr, lens)
    assert bool(torch.isfinite(s[[0, 4]]).all()) and bool(torch.isnan(s[1:4]).all())
    assert bool((grad[1:4] == 0).all())   # a NaN sample, no frame, digitally silent
    for b in (0, 4):
        nend = gc.nend_of(lens[b], sr)
        assert bool((grad[b, nend - 1:] == 0).all()) and float(grad[b, :nend - 1].abs().max()) > 0
    ref = metric(sr).scores(rows, lengths=lens)
    assert same_or_nan(s.float(), ref)
    # the loss: -mean over the scored rows
    est = rows.clone().requires_grad_(True)
    loss = metric(sr).loss(est, lengths=lens)
    assert abs(float(loss.detach()) + float(s[[0, 4]].mean())) <= 1e-12 * abs(float(loss.detach()))
    loss.backward()
    assert bool((est.grad[1:4] == 0).all()) and float(est.grad[0].abs().max()) > 0
    # no scored row: a zero with a zero gradient
    est = rows[1:4].clone().requires_grad_(True)
    loss = metric(sr).loss(est, lengths=lens[1:4])
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert est.grad.shape == (3, n) and bool((est.grad == 0).all())
    # rows of no samples: the scores, and an empty gradient
    est = rows[:, :0].clone().requires_grad_(True)
    s0 = metric(sr).differentiable_scores(est)
    assert s0.shape == (5,) and bool(torch.isnan(s0).all())
    s0.sum().backward()
    assert est.grad.shape == (5, 0)
    # a zero incoming gradient: zeros
    _, g0 = cpu_mode(rows[:1], sr, g=torch.zeros(1))
    assert bool((g0 == 0).all())
    fan = SRMR(sr, use_gpu=False)
    fan._fanout = object()   # (stands in for a metric built with devices=)
    for call in (fan.differentiable_scores, fan.loss):
        with pytest.raises(NotImplementedError, match="devices= is not supported with gradients"):
            call(rows)


@pytest.mark.parametrize("sr", gc.RATES)
def test_ascent(sr):
    """ASCENT_STEPS steps of x <- x + ASCENT_STEP |x|^2 dSRMR/dx raise SRMR at every step in CPU mode, where the
    step was chosen."""
    first, trace = gc.ascent(metric(sr), "cpu")
    print(f"cpu {sr}: SRMR {first:.4f} -> {' '.join(f'{v:.4f}' for v in trace)}")
    assert all(b > a for a, b in zip([first] + trace, trace))
