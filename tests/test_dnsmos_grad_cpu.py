"""DNSMOS with gradients without a GPU: CPU mode (float64 under torch's autograd) against the directly composed
float64 graph of tests/dnsmos_grad_cases.py and against a central difference, the recorded basis of the engine's
bar against a fresh measurement, the C entries (declared, exported, bound; every refusal answered on the host
before any launch), and the host layer's refusals, copies and pickles."""
import copy
import ctypes
import pickle
import subprocess

import numpy as np
import pytest
import torch

from fast_se_metrics.DNSMOS import DNSMOS as ReferenceNameDNSMOS
from fast_speech_enhancement_metrics_amd import DNSMOS, _build, _native

from . import contract
from . import dnsmos_cases as dc
from . import dnsmos_grad_cases as gc

ENTRIES = ("fsem_dnsmos_grad_scratch_floats", "fsem_dnsmos_grad_weights_floats", "fsem_dnsmos_grad_pack_weights_f32",
           "fsem_dnsmos_grad_f32", "fsem_dnsmos_grad_image_f32")


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.fixture(scope="module")
def metric():
    return DNSMOS(16000, weights=dc.WEIGHTS)


def test_entries_are_declared_exported_and_bound(lib):
    contract.entries_are_declared_exported_and_bound(lib, "fsem_dnsmos_", ENTRIES, others=())
    assert not set(ENTRIES) & set(_native.DNSMOS_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.DNSMOS_LIB], capture_output=True, text=True, check=True)
    assert not any(name in out.stdout for name in ENTRIES)   # (the forward's eight: tests/test_libraries_cpu.py)
    assert "dnsmos_grad.hip" in _build.SOURCES and "fsem_dnsmos_kernels.h" in _build.HEADERS
    assert _build.library("dnsmos").sources == ["dnsmos.hip"]
    assert ReferenceNameDNSMOS is DNSMOS and callable(DNSMOS.loss) and callable(DNSMOS.differentiable_scores)


def test_size_queries(lib):
    dn = _native.load_dnsmos()
    assert 4 * lib.fsem_dnsmos_grad_weights_floats() > dn.fsem_dnsmos_weights_bytes()   # (the forward's blob is its head)
    one = lib.fsem_dnsmos_grad_scratch_floats(1, 160000, 1)
    assert 4 * one > dn.fsem_dnsmos_min_workspace_bytes()
    prev = 0
    for P in range(1, 17):   # grows with the pass, by about one segment's buffers each time
        n = lib.fsem_dnsmos_grad_scratch_floats(3, 160000, P)
        assert prev < n <= P * one
        prev = n
    # the length does not enter; the batch does by one flag per row
    assert lib.fsem_dnsmos_grad_scratch_floats(3, 100, 4) == lib.fsem_dnsmos_grad_scratch_floats(3, 1 << 29, 4)
    assert 0 < lib.fsem_dnsmos_grad_scratch_floats(4096, 160000, 4) - lib.fsem_dnsmos_grad_scratch_floats(1, 160000, 4) <= 4096 + 64
    for B, L, P in ((0, 16000, 1), (-1, 16000, 1), (1, 0, 1), (1, (1 << 29) + 1, 1), (1, 16000, 0), (1, 16000, 17)):
        assert lib.fsem_dnsmos_grad_scratch_floats(B, L, P) == 0, (B, L, P)


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(256), None
    big = (1 << 29) + 4
    EINVAL = _native.FSEM_EINVAL
    shape = contract.each(EINVAL, dict(batch=0), dict(batch=-1), dict(length=0), dict(length=-4), dict(ld=15999),
                          dict(length=big, ld=big, ld_grad=big), dict(npass=0), dict(npass=17), dict(npass=-1))
    grad = contract.by_name(lib.fsem_dnsmos_grad_f32,
                            "deg batch length ld lengths weights g grad ld_grad raw scratch npass", null)
    ok = dict(deg=p, batch=3, length=16000, ld=16000, lengths=null, weights=p, g=p, grad=p, ld_grad=16000, raw=null,
              scratch=p, npass=4)
    contract.refusals(grad, ok, contract.nulled(EINVAL, "deg weights g grad scratch") + shape
                      + contract.each(EINVAL, dict(ld_grad=15999)))
    image = contract.by_name(lib.fsem_dnsmos_grad_image_f32, "deg batch length ld lengths weights g g_image scratch npass",
                             null)
    ok = dict(deg=p, batch=3, length=16000, ld=16000, lengths=null, weights=p, g=p, g_image=p, scratch=p, npass=4)
    contract.refusals(lambda **a: image(**{k: v for k, v in a.items() if k != "ld_grad"}), ok,
                      contract.nulled(EINVAL, "deg weights g g_image scratch") + shape)
    # the pack entry: null pointers, a null tensor, a blob one float short
    tensors = (ctypes.c_void_p * _native.DNSMOS_NUM_TENSORS)(*([256] * _native.DNSMOS_NUM_TENSORS))
    need = lib.fsem_dnsmos_grad_weights_floats()
    assert lib.fsem_dnsmos_grad_pack_weights_f32(None, p, need, null) == EINVAL
    assert lib.fsem_dnsmos_grad_pack_weights_f32(tensors, None, need, null) == EINVAL
    assert lib.fsem_dnsmos_grad_pack_weights_f32(tensors, p, need - 1, null) == _native.FSEM_EWORKSPACE
    assert lib.fsem_dnsmos_grad_pack_weights_f32(tensors, p, -1, null) == _native.FSEM_EWORKSPACE
    tensors[7] = None
    assert lib.fsem_dnsmos_grad_pack_weights_f32(tensors, p, need, null) == EINVAL


def test_cpu_mode_is_the_composed_float64_graph(metric):
    fx = dc.fixture("dnsmos_16k")
    row = fx.rows[0]
    want_s, want_g = gc.reference("dnsmos_16k", 0)
    est = row.double()[None].requires_grad_(True)   # (a float64 leaf: the gradient arrives unrounded)
    scores = metric.differentiable_scores(est)
    assert scores.dtype == torch.float64 and scores.shape == (1, 3)
    assert np.abs(scores.detach().numpy()[0] - want_s).max() <= 1e-12
    dc.assert_within(scores.detach(), fx.ref32[:1], dc.CPU_BAR, "CPU mode's float64 scores against ref32")
    loss = metric.loss(est)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and abs(float(loss.detach()) + want_s[2]) <= 1e-12
    loss.backward()
    err = gc.deviation(est.grad.numpy()[0], -want_g[2])
    print(f"CPU mode's loss gradient against the composed graph: {err:.2e}")
    assert err <= 1e-12
    for k, key in enumerate(DNSMOS.KEYS[:2]):
        est.grad = None
        metric.loss(est, key=key).backward()
        assert gc.deviation(est.grad.numpy()[0], -want_g[k]) <= 1e-12, key


def test_float64_gradient_against_a_central_difference():
    """x +- h d with d a random unit vector and h = 1e-6 times the row's RMS.  The scores are piecewise smooth
    (ReLU, pooling, the maximum over positions): the quotient is the derivative while no decision flips inside the
    step, which holds for a step of this length (a white perturbation of 1e-6 RMS in every sample, 380 times as
    long, flips one on this row and leaves 5e-3)."""
    row = dc.fixture("dnsmos_16k").rows[0].double()
    _, grad = gc.reference("dnsmos_16k", 0)
    d = torch.from_numpy(np.random.default_rng(5).standard_normal(row.numel()))
    d = d / d.norm()
    h = 1e-6 * float(row.square().mean().sqrt())
    with torch.no_grad():
        quot = ((gc.scores64(row + h * d) - gc.scores64(row - h * d)) / (2 * h)).numpy()
    for k, key in enumerate(DNSMOS.KEYS):
        dot = float(grad[k] @ d.numpy())
        print(f"{key}: <g, d> {dot:.9e}, central difference {quot[k]:.9e}, relative {abs(quot[k] - dot) / abs(dot):.2e}")
        assert abs(quot[k] - dot) <= 1e-5 * abs(dot), key


def test_the_recorded_basis_is_not_stale():
    """The emulation's deviation from float64 on one row and key, measured again, lies within a factor of 2 of
    the recorded maximum over the rows and keys: a guard against a stale file, not against rounding."""
    recorded = gc.basis()
    assert set(recorded) == {"basis", "basis_image"}
    fx = dc.fixture("dnsmos_16k")
    want = gc.reference("dnsmos_16k", 1, (1,))[1][0]   # row 1, BAK: the row and key of the recorded maximum
    _, got = gc.gradients(fx.rows[1], network=gc.emulated_network, keys=(1,))
    fresh = gc.deviation(got[0], want)
    print(f"basis: recorded {recorded['basis']:.3e}, row 1 BAK again {fresh:.3e}; basis_image {recorded['basis_image']:.3e}")
    assert recorded["basis"] / 2 <= fresh <= recorded["basis"] * 2
    assert 0 < recorded["basis"] < 0.5 and 0 < recorded["basis_image"] < 0.5


def test_conventions_in_cpu_mode(metric):
    src = dc.fixture("dnsmos_short").rows[0]
    rows = torch.stack([src[:2500], src[5000:7500]])   # (2500 samples: one segment of 57.7 periods)
    # a NaN row: NaN scores, a zero gradient row, the loss over the other row
    bad = rows.clone()
    bad[1, 100] = float("nan")
    est = bad.requires_grad_(True)
    scores = metric.differentiable_scores(est, lengths=[2500, 1250])
    assert bool(torch.isnan(scores[1]).all()) and bool(torch.isfinite(scores[0]).all())
    (-scores[0, 2]).backward()
    first = est.grad.clone()
    assert est.grad.dtype == torch.float32 and bool((est.grad[1] == 0).all()) and bool(est.grad[0].abs().max() > 0)
    # lengths: zeros past each length
    est = rows.clone().requires_grad_(True)
    loss = metric.loss(est, lengths=[2500, 1250])
    loss.backward()
    assert bool((est.grad[1, 1250:] == 0).all()) and bool(est.grad[1, :1250].abs().max() > 0)
    assert gc.deviation(est.grad[0].numpy(), first[0].numpy() / 2) <= 1e-6   # (the mean over two rows)
    # an all-NaN batch: a zero loss with a zero gradient
    allbad = torch.full_like(rows, float("nan")).requires_grad_(True)
    loss = metric.loss(allbad)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert allbad.grad.shape == rows.shape and bool((allbad.grad == 0).all())


def test_refusals(metric):
    rows = dc.fixture("dnsmos_short").rows[:1, :2500]
    with pytest.raises(ValueError, match="key"):
        metric.loss(rows, key="MOS")
    with pytest.raises(ValueError, match="sample_rate"):
        DNSMOS(8000, weights=dc.WEIGHTS).loss(rows)   # an 8 kHz metric must be told its rows' rate

    class Shards:   # (a fan-out needs GPUs to construct: stand in for one)
        pass

    m = DNSMOS(16000, weights=dc.WEIGHTS)
    m._fanout = Shards()
    with pytest.raises(NotImplementedError, match="devices"):
        m.differentiable_scores(rows)
    with pytest.raises(NotImplementedError, match="devices"):
        m.loss(rows)


def test_copies_and_pickles_drop_the_gradient_blob(metric):
    m = DNSMOS(16000, weights=dc.WEIGHTS)
    m._blobs[("grad", 0)] = m._blobs[0] = object()   # (stand-ins: the blobs live on a device)
    others = (copy.copy(m), copy.deepcopy(m), pickle.loads(pickle.dumps(m)))
    for other in others:
        assert other._blobs == {} and other.weights_file == m.weights_file
    rows = dc.fixture("dnsmos_short").rows[:1, 5000:7500].clone().requires_grad_(True)
    others[2].loss(rows).backward()
    assert bool(torch.isfinite(rows.grad).all()) and bool(rows.grad.abs().max() > 0)
