"""PITSDR without a GPU: the five C entries (declared, exported, bound; their queries and their refusals,
answered on the host before any launch), the package's CPU mode against the float64 statement of the
definition (tests/pitsdr_cases.py) in scores, assignment and gradients, the one-source corner against SDR,
SI-SDRi and the class API.

CPU mode computes in float64 (``_cpu.pitsdr``): its matrices are held to 1e-9 dB and its gradients to 1e-9
of the row's largest gradient.  ``scores`` returns float32 tensors by contract, which cannot carry 1e-9 dB:
they are checked to be exactly the float32 rounding of those float64 values."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import PITSDR, SDR, _build, _cpu, _native

from . import contract
from . import pitsdr_cases as pc
from . import sdr_cases as sc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("fsem_pitsdr_max_sources", "fsem_pitsdr_chunk", "fsem_pitsdr_sums_doubles", "fsem_pitsdr_f32",
           "fsem_pitsdr_grad_f32")


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.fixture(scope="module")
def metric():
    return PITSDR(16000)


def cpu64(metric, s, h, lengths=None, criterion="SI-SDR"):
    """CPU mode's float64 (si_mat, snr_mat, perm) and the class's float32 outputs, checked to be their rounding."""
    si, snr, perm = _cpu.pitsdr(s, h, lengths, metric.zero_mean, criterion)
    got = type(metric)(metric.sample_rate, zero_mean=metric.zero_mean, permutation=criterion).scores(
        s, h, lengths=lengths, return_matrix=True)
    assert [g.dtype for g in got] == [torch.float32] * 2 + [torch.int32] + [torch.float32] * 2
    assert torch.equal(got[2], perm)
    idx = perm.long()[:, None, :]
    for g, w in zip((got[0], got[1], got[3], got[4]), (si.gather(1, idx)[:, 0], snr.gather(1, idx)[:, 0], si, snr)):
        np.testing.assert_array_equal(g.numpy(), w.float().numpy())
    return si.gather(1, idx)[:, 0], snr.gather(1, idx)[:, 0], perm, si, snr


def test_entries_are_declared_exported_and_bound(lib):
    contract.entries_are_declared_exported_and_bound(lib, "fsem_pitsdr_", ENTRIES)
    assert "pitsdr.hip" in _build.SOURCES


def test_queries(lib):
    assert lib.fsem_pitsdr_max_sources() == 4 == PITSDR.MAX_SOURCES == _cpu.PITSDR_MAX_SOURCES
    for sr in (4000, 8000, 16000, 44100, 192000):
        C = lib.fsem_pitsdr_chunk(sr)
        assert C > 0 and C % 4 == 0
        for S, E in ((1, 1), (2, 2), (3, 2), (4, 4), (4, 1)):
            per = 2 * S + 2 * E + 2 * S * E  # ss, hh, s1, h1, sh, dd
            for L in (1, C - 1, C, C + 1, 10 * C, 1 << 29):
                assert lib.fsem_pitsdr_sums_doubles(S, E, L, sr) == per * (1 + -(-L // C)), (S, E, L, sr)
            assert lib.fsem_pitsdr_sums_doubles(S, E, 3 * C, sr) > lib.fsem_pitsdr_sums_doubles(S, E, 2 * C, sr)
    for S, E, L, sr in ((0, 1, 100, 16000), (5, 1, 100, 16000), (1, 0, 100, 16000), (4, 5, 100, 16000),
                        (1, 2, 100, 16000), (2, 3, 100, 16000), (2, 2, 0, 16000), (2, 2, (1 << 29) + 1, 16000),
                        (2, 2, 100, 3999), (2, 2, 100, 192001)):
        assert lib.fsem_pitsdr_sums_doubles(S, E, L, sr) == 0, (S, E, L, sr)
    assert lib.fsem_pitsdr_chunk(3999) == 0 and lib.fsem_pitsdr_chunk(192001) == 0


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(16), None
    big = (1 << 29) + 1
    EINVAL, ERATE, OK = _native.FSEM_EINVAL, _native.FSEM_ERATE, _native.FSEM_OK
    shapes = (dict(batch=-1), dict(S=0), dict(S=5), dict(E=0), dict(E=5), dict(S=2, E=3), dict(length=0),
              dict(ld=7999), dict(length=big, ld=big))
    fwd = contract.by_name(lib.fsem_pitsdr_f32, "src est batch S E length ld lengths sr zm crit sums si snr perm", null)
    ok = dict(src=p, est=p, batch=3, S=2, E=2, length=8000, ld=8000, lengths=null, sr=16000, zm=0, crit=1, sums=p,
              si=p, snr=p, perm=p)
    contract.refusals(fwd, ok, contract.nulled(EINVAL, "src est sums si snr perm")
                      + contract.each(EINVAL, *shapes, dict(crit=-1), dict(crit=3))
                      + contract.each(ERATE, dict(sr=3999), dict(sr=192001), dict(sr=0))
                      + contract.each(OK, dict(batch=0), dict(batch=0, lengths=p)))  # nothing launched
    bwd = contract.by_name(lib.fsem_pitsdr_grad_f32,
                           "src est batch S E length ld lengths zm sums g_si g_snr grad grad_ld", null)
    okg = dict(src=p, est=p, batch=3, S=2, E=2, length=8000, ld=8000, lengths=null, zm=0, sums=p, g_si=p, g_snr=p,
               grad=p, grad_ld=8000)
    contract.refusals(bwd, okg, contract.nulled(EINVAL, "src est sums g_si g_snr grad")
                      + contract.each(EINVAL, *shapes, dict(grad_ld=7999)) + contract.each(OK, dict(batch=0)))


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "S%d-E%d-n%d" % s)
@pytest.mark.parametrize("criterion", ["SI-SDR", "SNR", None])
def test_cpu_mode_against_the_definition(metric, shape, criterion):
    S, E, n = shape
    order = [(e + 1) % S for e in range(E)] if S == E else None  # estimates rotated against the sources
    s, h = pc.mixtures(2, S, E, n, order=order)
    want = pc.expected(s, h, criterion=criterion)
    if S == E and S > 1 and criterion is not None:
        assert want["perm"].tolist() == [order] * 2
    else:
        assert want["perm"].tolist() == [list(range(E))] * 2
    pc.assert_all_close(cpu64(metric, s, h, criterion=criterion), want, f"cpu mode {shape} {criterion}", pc.ATOL_CPU)


def test_cpu_mode_with_lengths(metric):
    s, h = pc.mixtures(4, 2, 2, 6000, seed=19, order=[1, 0])
    lens = [6000, 0, 4097, 3]
    want = pc.expected(s, h, lengths=lens, tie_ok=True)  # (the mixture without samples has no margin)
    assert (want["margin"][[0, 2, 3]] > pc.PERM_MARGIN).all()
    assert np.isnan(want["SI_mat"][1]).all() and want["perm"].tolist()[:3] == [[1, 0], [0, 1], [1, 0]]
    pc.assert_all_close(cpu64(metric, s, h, lengths=lens), want, "cpu mode, ragged batch", pc.ATOL_CPU)
    pc.assert_all_close(cpu64(metric, s, h, lengths=torch.tensor(lens)), want, "cpu mode, lengths as a tensor",
                        pc.ATOL_CPU)
    # the padding is never looked at
    s2, h2 = s.clone(), h.clone()
    s2[2, :, 4097:], h2[2, :, 4097:], h2[1] = float("nan"), float("inf"), float("nan")
    pc.assert_all_close(cpu64(metric, s2, h2, lengths=lens), want, "cpu mode, non-finite padding", pc.ATOL_CPU)


def test_cpu_mode_zero_mean_on_dc_rows():
    s, h = pc.dc_mixtures(*pc.mixtures(2, 2, 2, 5000, seed=13, order=[1, 0]))
    zm = PITSDR(16000, zero_mean=True)
    want = pc.expected(s, h, zero_mean=True)
    got = cpu64(zm, s, h)
    pc.assert_all_close(got, want, "cpu mode, zero_mean", pc.ATOL_CPU)
    plain = pc.expected(s, h)
    assert np.abs(plain["SI_mat"] - want["SI_mat"]).max() > 1.0  # (the offset matters without it)
    np.testing.assert_array_equal(plain["SNR_mat"], want["SNR_mat"])  # SNR is never centred


def test_cpu_mode_edge_mixtures(metric):
    s, h = pc.edge_mixtures()
    want = pc.expected(s, h, tie_ok=True)
    si, snr = want["SI"][:, 0], want["SNR"][:, 0]
    assert si[0] == math.inf and snr[0] == math.inf and math.isnan(si[1]) and snr[1] == -math.inf
    assert math.isnan(si[2]) and abs(snr[2]) < 1e-6 and math.isnan(si[3]) and math.isnan(snr[3])
    pc.assert_all_close(cpu64(metric, s, h), want, "cpu mode, edge mixtures", pc.ATOL_CPU)
    bad = s.clone()
    bad[0, 0, 5] = float("nan")
    got = metric.scores(bad, h, return_matrix=True)
    assert torch.isnan(got[0][0]).all() and torch.isnan(got[1][0]).all() and got[2][0].tolist() == [0]
    pc.assert_all_close(got, pc.expected(bad, h, tie_ok=True), "cpu mode, a NaN sample")
    empty = metric.scores(s[:, :, :0], h[:, :, :0])
    assert torch.isnan(empty[0]).all() and torch.isnan(empty[1]).all() and empty[0].shape == (4, 1)


def test_one_source_is_sdr(metric):
    c, n = sc.speech_rows(4, 8000, 16000)
    si, snr, perm, _, _ = cpu64(metric, c[:, None], n[:, None])
    assert not perm.any()
    got2d = metric.scores(c, n)
    assert got2d[0].shape == (4, 1) and torch.equal(got2d[0][:, 0], si[:, 0].float())
    ref = _cpu.sdr(c, n, 16000)
    np.testing.assert_allclose(si[:, 0].numpy(), ref[0].numpy(), rtol=0, atol=pc.ATOL_CPU)
    np.testing.assert_allclose(snr[:, 0].numpy(), ref[1].numpy(), rtol=0, atol=pc.ATOL_CPU)
    # SDR(...).scores' float32 against the float32 of the class: one rounding of values within 1e-9 dB
    cls = SDR(16000).scores(c, n)
    np.testing.assert_allclose(got2d[0][:, 0].numpy(), cls[0].numpy(), rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(got2d[1][:, 0].numpy(), cls[1].numpy(), rtol=2.0 ** -23, atol=0)
    want = sc.expected(c, n, 16000)
    pc.assert_scores_close(si[:, 0], want[0], "S = E = 1 SI-SDR against SDR's definition", pc.ATOL_CPU)
    pc.assert_scores_close(snr[:, 0], want[1], "S = E = 1 SNR against SDR's definition", pc.ATOL_CPU)
    cd, nd = sc.dc_rows(c, n)
    zm = PITSDR(16000, zero_mean=True)
    si0 = cpu64(zm, cd[:, None], nd[:, None])[0]
    np.testing.assert_allclose(si0[:, 0].numpy(), _cpu.sdr(cd, nd, 16000, True)[0].numpy(), rtol=0, atol=pc.ATOL_CPU)


def test_si_sdri_against_the_mixture(metric):
    s, h = pc.mixtures(2, 2, 2, 8000, seed=29, order=[1, 0])
    mix = s.sum(1)
    si, snr, perm, sdri = metric.scores(s, h, mixture=mix)
    assert perm.tolist() == [[1, 0], [1, 0]] and sdri.shape == (2, 2) and sdri.dtype == torch.float32
    want = pc.expected(s, h)
    base = pc.expected(s, mix[:, None], criterion=None)["SI_mat"][:, :, 0]  # SI-SDR(source i, mixture)
    pc.assert_scores_close(sdri, want["SI"] - base[:, [1, 0]], "SI-SDRi")
    out = metric.scores(s, h, mixture=mix, return_matrix=True)
    assert len(out) == 6 and torch.equal(out[5], sdri)
    assert out[3].shape == out[4].shape == (2, 2, 2) and out[3].dtype == out[4].dtype == torch.float32
    with pytest.raises(Exception, match="mixture"):
        metric.scores(s, h, mixture=mix[:, :100])


def test_permutation_rules(metric):
    s, h = pc.mixtures(1, 3, 3, 4000, seed=31)
    for order in ([1, 0, 2], [1, 2, 0], [2, 0, 1]):
        hp = h[:, order]
        for crit in ("SI-SDR", "SNR"):
            got = PITSDR(16000, permutation=crit).scores(s, hp)
            assert got[2][0].tolist() == order == pc.expected(s, hp, criterion=crit)["perm"][0].tolist()
        assert PITSDR(16000, permutation=None).scores(s, hp)[2][0].tolist() == [0, 1, 2]
    # equal means keep the first assignment: two identical estimates
    s2, h2 = pc.mixtures(1, 2, 2, 4000, seed=37)
    h2 = torch.stack([h2[:, 1], h2[:, 1]], 1)
    for crit in ("SI-SDR", "SNR"):
        want = pc.expected(s2, h2, criterion=crit, tie_ok=True)
        assert want["margin"][0] == 0.0 and want["perm"][0].tolist() == [0, 1]
        assert PITSDR(16000, permutation=crit).scores(s2, h2)[2][0].tolist() == [0, 1], crit
    # E < S and a NaN in the criterion matrix: the identity
    s3, h3 = pc.mixtures(1, 3, 2, 4000, seed=41)
    assert metric.scores(s3, h3)[2].tolist() == [[0, 1]]
    silent = torch.stack([h2[:, 0], torch.zeros_like(h2[:, 0])], 1)  # SI-SDR of a silent estimate is NaN
    assert metric.scores(s2, silent)[2].tolist() == [[0, 1]]
    assert PITSDR(16000, permutation="SNR").scores(s2, silent)[2].tolist() == [[1, 0]]


@pytest.mark.parametrize("key", ["SI-SDR", "SNR"])
@pytest.mark.parametrize("zero_mean", [False, True])
def test_loss_backward_against_the_definition(key, zero_mean):
    s, h = pc.mixtures(3, 2, 2, 3000, seed=43, order=[1, 0])
    if zero_mean:
        s, h = pc.dc_mixtures(s, h)
    lens = [3000, 1777, 2500]
    m = PITSDR(16000, zero_mean=zero_mean)
    est = h.double().requires_grad_(True)  # (CPU mode keeps float64 rows: the gradient arrives unrounded)
    loss = m.loss(s, est, lengths=lens, key=key)
    assert loss.dtype == torch.float64 and loss.dim() == 0
    loss.backward()
    want = pc.expected(s, h, lengths=lens, zero_mean=zero_mean)
    w = want["SI" if key == "SI-SDR" else "SNR"]
    assert abs(float(loss.detach()) + w.mean()) <= pc.ATOL_CPU
    g = torch.zeros(3, 2, 2, dtype=torch.float64)
    for b in range(3):
        for e in range(2):
            g[b, want["perm"][b, e], e] = -1.0 / 6
    zero = torch.zeros_like(g)
    grad, _ = pc.expected_grad(s, h, g if key == "SI-SDR" else zero, zero if key == "SI-SDR" else g, lengths=lens,
                               zero_mean=zero_mean)
    got = est.grad.numpy()
    scale = np.abs(grad).max(2, keepdims=True)
    err = float((np.abs(got - grad) / scale).max())
    print(f"cpu mode loss({key}, zero_mean={zero_mean}): worst gradient error {err:.3e} of the row's largest")
    assert err <= pc.RTOL_CPU
    for b, n in enumerate(lens):
        assert (got[b, :, n:] == 0).all()
    # a float32 leaf takes the same gradient, rounded once
    est32 = h.clone().requires_grad_(True)
    m.loss(s, est32, lengths=lens, key=key).backward()
    np.testing.assert_allclose(est32.grad.numpy(), got.astype(np.float32), rtol=2.0 ** -22, atol=0)


def test_scores_carry_the_gradient_and_perm_does_not(metric):
    s, h = pc.mixtures(2, 2, 2, 2000, seed=47)
    est = h.double().requires_grad_(True)
    si, snr, perm, si_mat, snr_mat = metric.scores(s, est, return_matrix=True)
    assert si.requires_grad and snr_mat.requires_grad and not perm.requires_grad
    g_si, g_snr = pc.incoming(2, 2, 2)
    (si_mat.double() * g_si).sum().backward(retain_graph=True)
    grad, _ = pc.expected_grad(s, h, g_si, torch.zeros_like(g_snr))
    # (through scores' float32 outputs the incoming gradient is float32: the float32 draws are exact)
    np.testing.assert_allclose(est.grad.numpy(), grad, rtol=0, atol=pc.RTOL_CPU * np.abs(grad).max())


def test_sources_are_constants(metric):
    s, h = pc.mixtures(1, 2, 2, 1000, seed=53)
    src = s.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="sources"):
        metric.scores(src, h)
    with pytest.raises(NotImplementedError, match="sources"):
        metric.loss(src, h.clone().requires_grad_(True))
    with torch.no_grad():
        assert metric.scores(src, h)[0].shape == (1, 2)  # (no graph asked for: they are detached)


def test_class_api(metric):
    import fast_se_metrics
    import fast_speech_enhancement_metrics_amd as pkg
    assert pkg.PITSDR is PITSDR and "PITSDR" in pkg.__all__
    assert fast_se_metrics.__all__ == ["STOI", "PESQ"] and not hasattr(fast_se_metrics, "PITSDR")
    assert PITSDR.KEYS == ("SI-SDR", "SNR") and PITSDR.higher_is_better is True
    assert metric.permutation == "SI-SDR" and metric.zero_mean is False and metric.sample_rate == 16000
    s, h = pc.mixtures(3, 2, 2, 1500, seed=59)
    with pytest.raises(NotImplementedError, match="lists"):
        metric([s[0]], [h[0]])
    with pytest.raises(NotImplementedError, match="lists"):
        metric.scores([s[0]], [h[0]])
    with pytest.raises(NotImplementedError, match="devices"):
        PITSDR(16000, devices=[0, 0])
    with pytest.raises(ValueError, match="permutation"):
        PITSDR(16000, permutation="SDR")
    for sr in (3999, 192001):
        with pytest.raises(NotImplementedError, match="sample rate"):
            PITSDR(sr)
    assert PITSDR(4000).sample_rate == 4000 and PITSDR(192000).sample_rate == 192000
    with pytest.raises(ValueError):
        metric.scores(s[:, :1], h)  # more estimates than sources
    with pytest.raises(ValueError):
        metric.scores(torch.zeros(1, 5, 2000), torch.zeros(1, 1, 2000))
    with pytest.raises(ValueError, match="key"):
        metric.loss(s, h, key="SegSNR")
    with pytest.raises(Exception, match="share"):
        metric.scores(s, h[:, :, :100])
    # the drop-in call: one dict per mixture, the means over its estimates; no graph is left
    lens = [1500, 700, 0]
    est = h.clone().requires_grad_(True)
    res = metric(s, est, lengths=lens)
    with torch.no_grad():
        si, snr, _ = metric.scores(s, est, lengths=lens)
    assert not si.requires_grad and si.grad_fn is None and est.grad is None
    assert [tuple(r) for r in res] == [PITSDR.KEYS] * 3
    for k, t in zip(PITSDR.KEYS, (si, snr)):
        np.testing.assert_array_equal(np.array([r[k] for r in res], np.float32), t.mean(1).numpy())
    assert all(isinstance(v, float) for r in res for v in r.values()) and math.isnan(res[2]["SI-SDR"])
