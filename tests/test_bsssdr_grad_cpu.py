"""BSSSDR with gradients without a GPU: the three C entries (declared, exported, bound; the state query; every
refusal answered on the host before any launch), the float64 statement of tests/bsssdr_grad_cases.py against the
scores' own statement and central differences, CPU mode (``_cpu.bsssdr64`` in float64 under torch's autograd)
against the statement in scores and gradients on every parity case, the conventions, and ``loss``."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from fast_se_metrics.SDR import SDR as ReferenceNameSDR
from fast_speech_enhancement_metrics_amd import BSSSDR, _build, _native

from . import bsssdr_cases as bc
from . import bsssdr_grad_cases as gc
from . import contract
from . import lsd_cases as lc

ENTRIES = ("fsem_bsssdr_state_floats", "fsem_bsssdr_state_f32", "fsem_bsssdr_grad_f32")


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


def test_entries_are_declared_exported_and_bound(lib):
    contract.entries_are_declared_exported_and_bound(lib, "fsem_bsssdr_", ENTRIES)
    assert not set(ENTRIES) & set(_native.BSSSDR_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.BSSSDR_LIB], capture_output=True, text=True, check=True)
    assert not any(name in out.stdout for name in ENTRIES)   # (the forward's six: tests/test_libraries_cpu.py)
    assert "bsssdr_grad.hip" in _build.SOURCES and "fsem_bsssdr_kernels.h" in _build.HEADERS
    sources = _build.library("bsssdr").sources
    assert "bsssdr_grad.hip" not in sources and "fsem_bsssdr_kernels.h" not in sources
    assert ReferenceNameSDR is BSSSDR and callable(ReferenceNameSDR.loss) and callable(ReferenceNameSDR.differentiable_scores)


def test_state_floats(lib):
    bs = _native.load_bsssdr()
    prev = 0
    for L in (1, 511, 4096, 16000, 32769, 160000):
        n1, n4 = lib.fsem_bsssdr_state_floats(1, L), lib.fsem_bsssdr_state_floats(4, L)
        assert 0 < n1 < n4 and n1 >= prev, L
        # the forward's workspace and one record of x [512] float64, coh and the flags per row
        assert 4 * n4 >= bs.fsem_bsssdr_workspace_bytes(4, L) + 4 * (8 * 512 + 16)
        prev = n1
    assert lib.fsem_bsssdr_state_floats(5, 16000) > lib.fsem_bsssdr_state_floats(4, 16000)
    assert lib.fsem_bsssdr_state_floats(1, 1 << 29) > 0
    for B, L in ((-1, 16000), (4, 0), (4, -1), (4, (1 << 29) + 1)):
        assert lib.fsem_bsssdr_state_floats(B, L) == 0, (B, L)
    assert lib.fsem_bsssdr_state_floats(0, 16000) == 0   # (no rows: nothing to keep)


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(256), None
    big = (1 << 29) + 4
    EINVAL, OK = _native.FSEM_EINVAL, _native.FSEM_OK
    shape = contract.each(EINVAL, dict(batch=-1), dict(length=0), dict(length=-4), dict(ld=15999),
                          dict(length=big, ld=big, grad_ld=big))
    fwd = contract.by_name(lib.fsem_bsssdr_state_f32, "ref deg batch length ld lengths load_diag sdr state", null)
    ok = dict(ref=p, deg=p, batch=3, length=16000, ld=16000, lengths=null, load_diag=0.0, sdr=p, state=p)
    contract.refusals(lambda **a: fwd(**{k: v for k, v in a.items() if k != "grad_ld"}), ok,
                      contract.nulled(EINVAL, "ref deg sdr state") + shape
                      + contract.each(EINVAL, dict(load_diag=float("nan")), dict(load_diag=float("inf")),
                                      dict(load_diag=float("-inf")))
                      + contract.each(OK, dict(batch=0), dict(batch=0, lengths=p)))
    bwd = contract.by_name(lib.fsem_bsssdr_grad_f32, "ref deg batch length ld lengths g state grad grad_ld", null)
    ok = dict(ref=p, deg=p, batch=3, length=16000, ld=16000, lengths=null, g=p, state=p, grad=p, grad_ld=16000)
    contract.refusals(bwd, ok, contract.nulled(EINVAL, "ref deg g state grad") + shape
                      + contract.each(EINVAL, dict(grad_ld=15999))
                      + contract.each(OK, dict(batch=0), dict(batch=0, lengths=p)))


def test_statement_scores_are_the_forward_statement():
    c, n = lc.speech_rows(3, 3000, seed=31)
    want, keep = bc.expected(c, n)
    for b in range(3):
        got = gc.expected_row(c[b].numpy(), n[b].numpy())[0]
        assert keep[b] and abs(got - want[b]) <= bc.STABLE_DB, (b, got, want[b])


@pytest.mark.parametrize("n", [300, 700])
def test_statement_against_central_differences(n):
    """The statement's gradient is that of the definition with the float32 quotients taken as smooth: central
    differences of the same definition with the quotient in float64 (h / |h| unrounded) agree to the size of
    that substitution."""
    c, y = lc.speech_rows(1, n, seed=31)
    s, h = c[0].numpy(), y[0].numpy()
    _, grad = gc.expected_row(s, h)
    sp = gc.quotients(s, h)[0]
    pad = np.zeros(gc.K - 1)
    r = np.correlate(np.concatenate([sp, pad]), sp, "valid")
    lag = np.arange(gc.K)
    Rinv = np.linalg.inv(r[np.abs(lag[:, None] - lag[None, :])])

    def smooth(hd):
        hq = hd / np.sqrt(np.sum(hd * hd))
        b = np.correlate(np.concatenate([hq, pad]), sp, "valid")
        coh = float(b @ Rinv @ b)
        return 10.0 * np.log10(coh / (1.0 - coh))

    rng = np.random.default_rng(n)
    scale = np.abs(grad).max()
    hd = h.astype(np.float64)
    for i in rng.choice(n, 8, replace=False):
        d = np.zeros(n)
        d[i] = 1e-6 * np.abs(hd).max()
        quot = (smooth(hd + d) - smooth(hd - d)) / (2 * d[i])
        print(f"n {n} coordinate {i}: gradient {grad[i]:.6e}, quotient - gradient {quot - grad[i]:.2e}")
        assert abs(quot - grad[i]) <= 1e-3 * scale


def cpu_mode(name, g=None):
    """(scores [B], gradient [B, L]) of CPU mode on a named case for the incoming gradient g (ones)."""
    c, n, sr, lens, diag = gc.rows(name)
    m = BSSSDR(sr)
    m.load_diag = diag
    est = n.double().requires_grad_(True)   # (a float64 leaf: the gradient arrives unrounded)
    sdr = m.differentiable_scores(c, est, sr, lengths=None if lens is None else list(lens))
    assert sdr.dtype == torch.float64 and sdr.shape == (c.shape[0],)
    g = torch.ones(c.shape[0]) if g is None else g
    (sdr * g.double()).sum().backward()
    return sdr.detach().numpy(), est.grad.numpy()


@pytest.mark.parametrize("name", gc.PARITY)
def test_cpu_mode_against_the_statement(name):
    want_s, want_g = gc.expected(name)
    scored = np.isfinite(want_s)   # (the one-sample row of ``edges`` is a zero sample: a silent clean row, NaN)
    assert np.isfinite(want_g).all() and scored.sum() >= len(want_s) - 1
    scores, grad = cpu_mode(name)
    assert (np.isnan(scores) == ~scored).all() and np.abs(scores - want_s)[scored].max() <= bc.ATOL_DB
    err = gc.row_errors(grad, want_g)
    print(f"cpu mode {name}: scores {' '.join(f'{v:.2f}' for v in want_s)} dB; gradient row errors "
          f"{' '.join(f'{v:.2e}' for v in err)}; bar {gc.RTOL_CPU:.2e}; float32 autograd "
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
    assert gc.BAR == 4 * gc.MEASURED <= gc.BAR_LIMIT
    assert gc.RTOL_CPU == 4 * gc.MEASURED_CPU <= gc.RTOL_CPU_LIMIT


def test_conventions_in_cpu_mode():
    m = BSSSDR(16000)
    c, n, _, _, _ = gc.rows("speech")
    c, n = c[:, :3000], n[:, :3000]
    est = n.double().requires_grad_(True)
    good = m.differentiable_scores(c, est)
    good.sum().backward()
    # a non-finite sample, in either operand: NaN and a zero row, the other rows bitwise unchanged
    for where in ("estimate", "clean"):
        cb, nb = c.clone(), n.clone()
        (nb if where == "estimate" else cb)[1, 1000] = float("nan") if where == "estimate" else float("inf")
        bad = nb.double().requires_grad_(True)
        sdr = m.differentiable_scores(cb, bad)
        assert bool(torch.isnan(sdr[1])) and bool(torch.isfinite(sdr[[0, 2, 3]]).all())
        sdr[[0, 2, 3]].sum().backward()
        assert (bad.grad[1] == 0).all()
        contract.assert_bitwise(bad.grad[[0, 2, 3]], est.grad[[0, 2, 3]], where)
        contract.assert_bitwise(sdr[[0, 2, 3]], good[[0, 2, 3]], where)
    # a silent estimate: -80 and a zero row; a silent clean row: NaN and a zero row; identical rows: +80, finite
    cb, nb = c.clone(), n.clone()
    nb[0], cb[1], nb[2] = 0.0, 0.0, c[2]
    nb[3] = n[3] * (1e-7 / float(n[3].double().norm()))   # the estimate's norm below its clamp
    e2 = nb.double().requires_grad_(True)
    sdr = m.differentiable_scores(cb, e2)
    sdr[[0, 2, 3]].sum().backward()
    sdr = sdr.detach()
    assert float(sdr[0]) == -80.0 and (e2.grad[0] == 0).all()
    assert bool(torch.isnan(sdr[1])) and (e2.grad[1] == 0).all()
    # (coh is the sum of squares of float32 quotients, 1 up to 1e-7: +80 at or above 1 - 1e-8, else 70 dB and up)
    assert bc.HIGH_DB <= float(sdr[2]) <= 80.0 + 1e-6 and bool(torch.isfinite(e2.grad[2]).all())
    print(f"identical rows: {float(sdr[2]):.2f} dB, max |g| {float(e2.grad[2].abs().max()):.3e}")
    s3, g3 = gc.expected_row(cb[3].numpy(), nb[3].numpy())
    assert gc.quotients(cb[3].numpy(), nb[3].numpy())[3]
    assert abs(float(sdr[3]) - s3) <= bc.ATOL_DB and gc.row_errors(e2.grad[3:4].numpy(), g3[None]).max() <= gc.RTOL_CPU
    # lengths: zeros past each length, each row as the row alone
    lens = [3000, 700, 255, 1]
    e3 = n.double().requires_grad_(True)
    sdr = m.differentiable_scores(c, e3, lengths=lens)
    sdr.sum().backward()
    for b, k in enumerate(lens):
        s, g = gc.expected_row(c[b, :k].numpy(), n[b, :k].numpy())
        assert (e3.grad[b, k:] == 0).all() and bool(torch.isfinite(e3.grad[b]).all())
        assert abs(float(sdr[b].detach()) - s) <= bc.ATOL_DB
        assert gc.row_errors(e3.grad[b:b + 1, :k].numpy(), g[None]).max() <= gc.RTOL_CPU
    # a batch of no samples (NaN scores, an empty gradient), and no rows
    empty = n[:, :0].clone().requires_grad_(True)
    sdr = m.differentiable_scores(c[:, :0], empty)
    assert sdr.shape == (4,) and bool(torch.isnan(sdr).all())
    (sdr.nan_to_num().sum() + empty.sum()).backward()
    assert empty.grad.shape == (4, 0)
    assert m.differentiable_scores(c[:0], n[:0].clone().requires_grad_(True)).shape == (0,)


def test_loss():
    m = BSSSDR(16000)
    c, n, _, _, _ = gc.rows("speech")
    want_s, want_g = gc.expected("speech")
    est = n.clone().requires_grad_(True)
    loss = m.loss(c, est)
    assert loss.dtype == torch.float64 and loss.dim() == 0
    assert abs(float(loss.detach()) + want_s.mean()) <= bc.ATOL_DB   # higher is better: the loss is -mean
    loss.backward()
    assert est.grad.dtype == torch.float32
    assert gc.row_errors(est.grad.double().numpy(), -want_g / 4).max() <= 2.0 ** -22
    # the mean is over the rows with a finite score
    bad = n.clone()
    bad[2, 100] = float("nan")
    est = bad.requires_grad_(True)
    loss = m.loss(c, est)
    assert abs(float(loss.detach()) + want_s[[0, 1, 3]].mean()) <= bc.ATOL_DB
    loss.backward()
    assert (est.grad[2] == 0).all()
    assert gc.row_errors(est.grad[[0, 1, 3]].double().numpy(), -want_g[[0, 1, 3]] / 3).max() <= 2.0 ** -22
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
        BSSSDR(8000).loss(c, n)   # an 8 kHz metric must be told its rows' rate
    fixed = BSSSDR(16000)
    fixed.zero_mean = True
    with pytest.raises(NotImplementedError, match="zero_mean"):
        fixed.loss(c, n)
    half = n[:, :2000].to(torch.bfloat16).requires_grad_(True)
    m.loss(c[:, :2000], half).backward()
    assert half.grad.dtype == torch.bfloat16 and bool(torch.isfinite(half.grad.float()).all())


def test_it_trains_in_cpu_mode():
    first, trace = gc.ascent(BSSSDR(16000), "cpu")
    print(f"SDR {first:.3f} -> {' '.join(f'{v:.3f}' for v in trace)}")
    assert all(b > a for a, b in zip([first] + trace, trace)) and trace[-1] >= first + 3.0


def test_devices_are_refused():
    class Shards:   # (a fan-out needs GPUs to construct: stand in for one)
        pass

    m = BSSSDR(16000)
    m._fanout = Shards()
    c, n, _, _, _ = gc.rows("speech")
    with pytest.raises(NotImplementedError, match="devices"):
        m.differentiable_scores(c, n)
    with pytest.raises(NotImplementedError, match="devices"):
        m.loss(c, n)
