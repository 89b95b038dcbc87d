"""STOI with gradients without a GPU: the three C entries (declared, exported, bound; the state query; every
refusal answered on the host before any launch), CPU mode (``_cpu.stoi`` in float64 under torch's autograd)
against the reference of tests/stoi_grad_cases.py in scores and gradients, the reference itself against central
differences, and the class API.

CPU mode is held to 1e-12 in the scores and to 1e-9 of the row's largest gradient element.  The central
differences use one step for every set, FD_EPS = 5e-4 along unit directions over the whole batch: measured
here, the quotient is within 4.5e-6 of <g, d> (relative) at that step and within 1.2e-6 at half of it, so
halving moves it by less than FD_BAR = 1e-5, the bar of the check."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import STOI, _build, _cpu, _native

from . import contract
from . import stoi_grad_cases as gc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("fsem_stoi_state_floats", "fsem_stoi_state_f32", "fsem_stoi_grad_f32")
NAMES = [s[0] for s in gc.SETS]


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


def test_entries_are_declared_exported_and_bound(lib):
    old = {"fsem_stoi_workspace_bytes", "fsem_stoi_f32", "fsem_stoi_tob_f32"}
    contract.entries_are_declared_exported_and_bound(lib, "fsem_stoi_", ENTRIES, old)
    assert "stoi_grad.hip" in _build.SOURCES and "fsem_stoi.h" in _build.HEADERS


def test_state_floats(lib):
    for sr in (8000, 10000, 16000, 48000):
        prev_l = 0
        for L in (sr // 10, sr, 4 * sr, 10 * sr):
            n1, n4 = lib.fsem_stoi_state_floats(1, L, sr), lib.fsem_stoi_state_floats(4, L, sr)
            assert 0 < n1 < n4 and n1 > prev_l, (sr, L)
            assert 4 * n1 >= lib.fsem_stoi_workspace_bytes(1, L, sr)  # the state's head is the forward's workspace
            prev_l = n1
    for B, L, sr in ((4, 0, 16000), (4, -1, 16000), (4, (1 << 29) + 4, 16000), (4, 16000, 44101), (4, 16000, 0), (-1, 16000, 16000)):
        assert lib.fsem_stoi_state_floats(B, L, sr) == 0, (B, L, sr)


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(256), None
    big = (1 << 29) + 4
    EINVAL, ERATE, OK = _native.FSEM_EINVAL, _native.FSEM_ERATE, _native.FSEM_OK
    shapes = (dict(batch=-1), dict(length=0), dict(length=-4), dict(ld=15999), dict(length=big, ld=big))
    fwd = contract.by_name(lib.fsem_stoi_state_f32, "ref deg batch length ld lengths sr s e seg state", null)
    ok = dict(ref=p, deg=p, batch=3, length=16000, ld=16000, lengths=null, sr=16000, s=p, e=p, seg=p, state=p)
    contract.refusals(fwd, ok, contract.nulled(EINVAL, "ref deg s e state") + contract.each(EINVAL, *shapes)
                      + contract.each(ERATE, dict(sr=44101), dict(sr=0)))
    contract.refusals(fwd, dict(ok, batch=0), contract.each(  # nothing launched
        OK, dict(), dict(lengths=p), dict(seg=null), dict(sr=10000), dict(sr=48000)))
    bwd = contract.by_name(lib.fsem_stoi_grad_f32, "deg batch length ld lengths sr state gs ge grad grad_ld", null)
    okg = dict(deg=p, batch=3, length=16000, ld=16000, lengths=null, sr=16000, state=p, gs=p, ge=p, grad=p,
               grad_ld=16000)
    contract.refusals(bwd, okg, contract.nulled(EINVAL, "deg state gs ge grad")
                      + contract.each(EINVAL, *shapes, dict(grad_ld=15999))
                      + contract.each(ERATE, dict(sr=44101), dict(sr=0))
                      + contract.each(OK, dict(batch=0), dict(batch=0, lengths=p, sr=8000)))


def test_case_shapes():
    assert gc.segments("16k") == [12, 46, 2, 44] and min(gc.segments("8k")) > 0
    assert [s == 0 for s in gc.segments("10k")] == [False, False, True, False]   # row 2: no 30-frame segment
    assert [s == 0 for s in gc.segments("48k")] == [False, False, True, False]
    assert gc.segments(gc.LONG[0])[0] + 31 >= 288   # more than 256 segments: two forward segment blocks


def cpu_mode(name, lengths=None, g=None):
    """(scores [B, 2], gradient [B, L]) of CPU mode on a named set for incoming (g_s, g_e)."""
    c, n, sr = gc.rows(name)
    est = n.double().requires_grad_(True)   # (a float64 leaf: the gradient arrives unrounded)
    s, e = STOI(sr).differentiable_scores(c, est, sr, lengths=lengths)
    assert s.dtype == e.dtype == torch.float64 and s.shape == e.shape == (c.shape[0],)
    g_s, g_e = g if g is not None else gc.incoming(c.shape[0])
    live = ~torch.isnan(s)
    if bool(live.any()):
        (s[live] * g_s.double()[live] + e[live] * g_e.double()[live]).sum().backward()
    grad = est.grad.numpy() if est.grad is not None else np.zeros(tuple(n.shape))
    return torch.stack([s, e], 1).detach().numpy(), grad, (g_s.numpy(), g_e.numpy())


@pytest.mark.parametrize("name", NAMES + ["zero"])
def test_cpu_mode_against_the_reference(name):
    want = gc.expected(name)
    scores, grad, (g_s, g_e) = cpu_mode(name)
    np.testing.assert_allclose(scores, want["scores"], rtol=0, atol=gc.ATOL_SCORE_CPU, equal_nan=True)
    c, n, sr = gc.rows(name)
    direct = torch.stack(_cpu.stoi(gc.resample64(c, sr), gc.resample64(n, sr)), 1).numpy()
    np.testing.assert_allclose(scores, direct, rtol=0, atol=gc.ATOL_SCORE_CPU, equal_nan=True)
    err = gc.row_errors(grad, gc.combine(want, g_s, g_e))
    print(f"cpu mode {name}: worst gradient error {err.max():.3e} of the row's largest")
    assert np.isfinite(grad).all() and err.max() <= gc.RTOL_CPU
    for b, seg in enumerate(gc.segments(name)):
        if seg == 0:
            assert np.isnan(scores[b]).all() and (grad[b] == 0).all()
    if name == "zero":
        assert (scores[1] == 0).all() and (grad[1] == 0).all() and np.abs(grad[0]).max() > 0


def test_cpu_mode_with_lengths():
    lens = gc.RAGGED_LENGTHS
    want = gc.expected("16k", tuple(lens))
    scores, grad, (g_s, g_e) = cpu_mode("16k", lengths=lens)
    np.testing.assert_allclose(scores, want["scores"], rtol=0, atol=gc.ATOL_SCORE_CPU, equal_nan=True)
    assert gc.row_errors(grad, gc.combine(want, g_s, g_e)).max() <= gc.RTOL_CPU
    for b, n in enumerate(lens):
        assert (grad[b, n:] == 0).all()
    assert np.isnan(scores[3]).all() and (grad[3] == 0).all() and np.abs(grad[1]).max() > 0


def test_a_row_with_a_non_finite_sample_gets_no_gradient():
    c, n, sr = gc.rows("16k")
    bad = n.clone()
    bad[1, 5000] = float("nan")
    est = bad.double().requires_grad_(True)
    s, e = STOI(sr).differentiable_scores(c, est, sr)
    (s[[0, 2, 3]].sum() + e[[0, 2, 3]].sum()).backward()
    want = gc.expected("16k")
    ones = np.ones(4)
    assert (est.grad[1] == 0).all()
    assert gc.row_errors(est.grad.numpy()[[0, 2, 3]], gc.combine(want, ones, ones)[[0, 2, 3]]).max() <= gc.RTOL_CPU


@pytest.mark.parametrize("name", NAMES)
def test_reference_against_central_differences(name):
    c, n, sr = gc.rows(name)
    want = gc.expected(name)
    segs = gc.segments(name)
    c10 = [gc.resample64(c[b:b + 1], sr) if segs[b] > 0 else None for b in range(4)]

    def f(est):  # sum over the scored rows of STOI_b + ESTOI_b, float64, no autograd
        tot = 0.0
        with torch.no_grad():
            for b in range(4):
                if c10[b] is not None:
                    s, e = _cpu.stoi(c10[b], gc.resample64(est[b:b + 1], sr))
                    tot += float(s[0]) + float(e[0])
        return tot

    g = torch.from_numpy(want["gs"] + want["ge"])
    gen = torch.Generator().manual_seed(5)
    y = n.double()
    for k in range(3):
        d = torch.randn(n.shape, generator=gen, dtype=torch.float64)
        d /= d.norm()
        dot = float((g * d).sum())
        q = [(f(y + eps * d) - f(y - eps * d)) / (2 * eps) for eps in (gc.FD_EPS, gc.FD_EPS / 2)]
        print(f"{name} direction {k}: <g, d> = {dot:.6e}, quotient - <g, d> = {q[0] - dot:.2e} at eps {gc.FD_EPS:g}, "
              f"{q[1] - dot:.2e} at half of it")
        assert abs(q[0] - q[1]) <= gc.FD_BAR * abs(dot)   # the step is in the quotient's flat range
        assert abs(q[0] - dot) <= gc.FD_BAR * abs(dot)


def test_the_float32_yardstick_and_the_bar():
    worst = max(float(v.max()) for v in gc.yardstick().values())
    print(f"float32 restatement against the float64 reference: worst row error {worst:.3e}; bar {gc.bar():.3e}")
    assert 1e-6 < worst < 5e-5 and gc.bar() == gc.BAR_FACTOR * worst   # (a wrong adjoint is off by 1e-2 or more)


def test_class_api():
    m = STOI(16000)
    c, n, sr = gc.rows("16k")
    with pytest.raises(ValueError, match="key"):
        m.loss(c, n, 16000, key="PESQ")
    src = c.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="constants"):
        m.differentiable_scores(src, n, 16000)
    with pytest.raises(NotImplementedError, match="constants"):
        m.loss(src, n.clone().requires_grad_(True), 16000)
    with torch.no_grad():
        assert m.differentiable_scores(src, n, 16000)[0].shape == (4,)   # (no graph asked for)
    with pytest.raises(ValueError, match="sample_rate"):
        m.loss(c, n)   # a 16 kHz metric must be told its rows' rate
    # loss: minus the mean over the rows that have a segment, float64 in CPU mode
    want = gc.expected("10k")
    c10, n10, _ = gc.rows("10k")
    est = n10.clone().requires_grad_(True)
    for key, col in (("STOI", 0), ("ESTOI", 1)):
        est.grad = None
        loss = STOI(10000).loss(c10, est, key=key)
        assert loss.dtype == torch.float64 and loss.dim() == 0
        assert abs(float(loss.detach()) + np.nanmean(want["scores"][:, col])) <= 1e-12
        loss.backward()
        w = -want["gs" if col == 0 else "ge"] / 3
        assert est.grad.dtype == torch.float32 and (est.grad[2] == 0).all()
        np.testing.assert_allclose(est.grad.numpy(), w.astype(np.float32), rtol=2.0 ** -22, atol=1e-12)
    assert float(STOI(10000).loss(c10, n10).detach()) == float(STOI(10000).loss(c10, n10, key="ESTOI").detach())
    # no scored row: the warning, and a zero that carries a zero gradient
    short = n[:, :3000].clone().requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="Not enough non-silent frames"):
        loss = m.loss(c[:, :3000], short, 16000)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert (short.grad == 0).all() and short.grad.shape == short.shape
    # scores() stays detached; half precision estimates get their gradient in their own dtype
    est = n.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s, e = m.scores(c, est, 16000)
    assert s.grad_fn is None and e.grad_fn is None and not s.requires_grad
    half = n.to(torch.bfloat16).requires_grad_(True)
    m.loss(c, half, 16000).backward()
    assert half.grad.dtype == torch.bfloat16 and bool(torch.isfinite(half.grad.float()).all())


def test_devices_are_refused():
    class Shards:   # (a fan-out needs GPUs to construct: stand in for one)
        pass

    m = STOI(16000)
    m._fanout = Shards()
    c, n, _ = gc.rows("16k")
    with pytest.raises(NotImplementedError, match="devices"):
        m.differentiable_scores(c, n, 16000)
    with pytest.raises(NotImplementedError, match="devices"):
        m.loss(c, n, 16000)
