"""PESQ with gradients without a GPU: the cases' decision margins, the float64 reference of
tests/pesq_grad_cases.py against central differences and against ``_cpu.pesq``, CPU mode
(``_cpu.pesq_differentiable`` in float64 under torch's autograd) against the reference in scores and gradients,
``loss`` with both keys, every refusal, and the three C entries (declared, exported, bound; the state query;
every refusal answered on the host before any launch).

CPU mode is held to 1e-12 in the scores and to 1e-9 of the row's largest gradient element.  The central
differences run along random directions scaled to the row's norm at steps 1e-5 and 1e-6 (both printed); at 1e-4
and above the quotient crosses the jump at a = 3, where the function is discontinuous, and stops converging."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import PESQ, _build, _cpu, _native

from . import contract
from . import pesq_grad_cases as gc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("fsem_pesq_state_floats", "fsem_pesq_state_f32", "fsem_pesq_grad_f32")
NAMES = ["main", "short", "long", "odd", "zero", "bad"]


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


def test_entries_are_declared_exported_and_bound(lib):
    contract.entries_are_declared_exported_and_bound(lib, "fsem_pesq_", ENTRIES, None)  # (the others: test_abi_cpu)
    assert "pesq_grad.hip" in _build.SOURCES and "pesq_grad.hip" not in _build.SOURCE_FLAGS


def test_state_floats(lib):
    prev = 0
    for L in (5376, 16000, 64000, 160000):
        n1, n4 = lib.fsem_pesq_state_floats(1, L), lib.fsem_pesq_state_floats(4, L)
        assert 0 < n1 < n4 and n1 > prev, L
        assert 4 * n1 >= lib.fsem_pesq_workspace_bytes(1, L)   # the state's head is the forward's workspace
        prev = n1
    assert 4 * lib.fsem_pesq_state_floats(1, 160000) < 1.8e6   # (1.69 MB per 10 s row)
    for B, L in ((4, 0), (4, -1), (4, (1 << 29) + 4), (-1, 16000)):
        assert lib.fsem_pesq_state_floats(B, L) == 0, (B, L)


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(256), None
    big = (1 << 29) + 4
    EINVAL, OK = _native.FSEM_EINVAL, _native.FSEM_OK
    shapes = (dict(batch=-1), dict(length=0), dict(length=-4), dict(ld=15999), dict(length=big, ld=big))
    fwd = contract.by_name(lib.fsem_pesq_state_f32, "ref deg batch length ld lengths mos dist state", null)
    ok = dict(ref=p, deg=p, batch=3, length=16000, ld=16000, lengths=null, mos=p, dist=p, state=p)
    contract.refusals(fwd, ok, contract.nulled(EINVAL, "ref deg mos state") + contract.each(EINVAL, *shapes) + [
        (dict(length=4000, ld=4000), _native.FSEM_ESHORT)])  # under 20 frames without lengths, as fsem_pesq_wb_f32
    # nothing launched
    contract.refusals(fwd, dict(ok, batch=0), contract.each(OK, dict(), dict(lengths=p), dict(dist=null)))
    bwd = contract.by_name(lib.fsem_pesq_grad_f32, "deg batch length ld lengths state gm gs ga grad grad_ld", null)
    okg = dict(deg=p, batch=3, length=16000, ld=16000, lengths=null, state=p, gm=p, gs=p, ga=p, grad=p, grad_ld=16000)
    contract.refusals(bwd, okg, contract.nulled(EINVAL, "deg state gm grad")
                      + contract.each(EINVAL, *shapes, dict(grad_ld=15999))
                      + contract.each(OK, dict(batch=0), dict(batch=0, lengths=p, gs=null, ga=null)))


def test_the_cases_score_what_they_should():
    np.testing.assert_allclose(gc.expected("main")["scores"][:, 0], [1.48, 1.15, 1.84, 4.15], atol=0.005)
    np.testing.assert_allclose(gc.expected("short")["scores"][:, 0], [1.03, 1.03, 1.26, 2.90], atol=0.005)
    assert gc.frames_of(gc.MAIN[1]) == 62 and gc.frames_of(gc.SHORT[1]) == 20 and gc.frames_of(gc.LONG[1]) > 3 * 48
    assert gc.scored("main", tuple(gc.RAGGED_LENGTHS)) == [True, True, True, False]
    assert gc.scored("zero") == gc.scored("bad") == [True, False, True, True]


@pytest.mark.parametrize("name,lengths", [("main", None), ("short", None), ("long", None), ("odd", None),
                                          ("main", tuple(gc.RAGGED_LENGTHS))])
def test_the_cases_stay_clear_of_the_decisions(name, lengths):
    """The decisions are constants of the function, so a float32 evaluation that takes one differently from
    float64 differs by that element's whole contribution: the cases stay clear of the two thresholds where that
    can happen, by the float64 reference alone.  The other decisions need no guard, because the value and the
    gradient contribution vanish at the threshold:
      - the dead zone: d = sign(d0) max(|d0| - m, 0) and its derivative's factor in the symmetric term 2 w^2 d
        are 0 at |d0| = m (in the asymmetric term d multiplies a, and |w d a| is continuous through d = 0);
      - p <= thr in the loudness: (0.5 + 0.5 p / thr)^e - 1 is 0 at p = thr, and the band's loudness enters
        through d alone;
      - the audible masks (> thr, > 100 thr): the masked powers are of order thr (1e2 ... 1e4) beside frame
        and band sums of order 1e7 and the additive 5e3 / 1e5 / 1000 terms, so a flipped element moves a ratio
        by ~1e-5 of itself, and through the ratios' small sensitivities;
      - the clamps' edges (0.01 .. 100, 3e-4 .. 5, 12, 45, 1e-20): continuous in value; a frame at a cap
        contributes a gradient of either side's size, bounded by the frame's own share."""
    want = gc.expected(name, lengths)
    print(f"{name} {lengths}: smallest |a - 3| / 3 = {want['a_margin']:.3e}, silent-frame margin {want['silent_margin']:.3e}")
    assert want["a_margin"] >= gc.MARGIN_ASYM
    assert want["silent_margin"] >= gc.MARGIN_SILENT


@pytest.mark.parametrize("name", ["main", "short"])
def test_reference_against_central_differences(name):
    c, d = gc.rows(name)
    want = gc.expected(name)
    gen = torch.Generator().manual_seed(5)
    for b in range(c.shape[0]):
        x = d[b].double()

        def f(v):
            with torch.no_grad():
                return float(gc.restated(c[b], v, torch.float64)[0])

        for k in range(2):
            u = torch.randn(x.shape, generator=gen, dtype=torch.float64)
            u *= x.norm() / u.norm()
            dot = float((torch.tensor(want["gm"][b]) * u).sum())
            q = [(f(x + eps * u) - f(x - eps * u)) / (2 * eps) for eps in gc.FD_STEPS]
            print(f"{name} row {b} direction {k}: <g, u> = {dot:.6e}, quotient - <g, u> = "
                  + ", ".join(f"{v - dot:.2e} at step {eps:g}" for v, eps in zip(q, gc.FD_STEPS)))
            assert min(abs(v - dot) for v in q) <= gc.FD_BAR * abs(dot)


@pytest.mark.parametrize("name", ["main", "short", "long", "odd"])
def test_restatement_in_float64_is_the_package_function(name):
    c, d = gc.rows(name)
    want = gc.expected(name)
    np.testing.assert_allclose(want["scores"][:, 0], _cpu.pesq(c, d).numpy(), rtol=0, atol=1e-12)
    sd, ad = _cpu.pesq_distances(c, d)
    np.testing.assert_allclose(want["scores"][:, 1:], torch.stack([sd, ad], 1).numpy(), rtol=1e-12, atol=0)
    x = d.double()
    for k in gc.KEYS:   # <g, x> = 0: the score does not depend on the scale of x
        g = torch.tensor(want[k])
        cos = (g * x).sum(1).abs() / (g.norm(dim=1) * x.norm(dim=1)).clamp(min=1e-300)
        assert float(cos.max()) < 1e-12, (k, cos)


def cpu_mode(name, lengths=None):
    """(scores [B, 3], gradients {key: [B, L]}) of CPU mode on a named case."""
    c, d = gc.rows(name)
    grads = {}
    for i, k in enumerate(gc.KEYS):
        est = d.double().requires_grad_(True)   # (a float64 leaf: the gradient arrives unrounded)
        out = PESQ(16000)._differentiable(c, est, None, lengths)
        assert out[0].dtype == torch.float64 and out[0].shape == (c.shape[0],)
        live = torch.isfinite(out[i].detach())
        if bool(out[i].requires_grad):
            out[i][live].sum().backward()
        grads[k] = est.grad.numpy() if est.grad is not None else np.zeros(tuple(d.shape))
        scores = torch.stack(out[:3], 1).detach().numpy()
    return scores, grads


@pytest.mark.parametrize("name", NAMES)
def test_cpu_mode_against_the_reference(name):
    want = gc.expected(name)
    scores, grads = cpu_mode(name)
    live = np.array(gc.scored(name))
    np.testing.assert_allclose(scores[live, 0], want["scores"][live, 0], rtol=0, atol=gc.ATOL_SCORE_CPU)
    np.testing.assert_allclose(scores[live, 1:], want["scores"][live, 1:], rtol=gc.ATOL_SCORE_CPU, atol=0)
    c, d = gc.rows(name)
    np.testing.assert_allclose(scores[live, 0], PESQ(16000).scores(c, d).numpy()[live], rtol=0, atol=gc.ATOL_SCORE_CPU)
    assert not np.isfinite(scores[~live, 0]).any()
    for k in gc.KEYS:
        err = gc.row_errors(grads[k], want[k])
        print(f"cpu mode {name} {k}: worst gradient error {err.max():.3e} of the row's largest")
        assert np.isfinite(grads[k]).all() and err.max() <= gc.RTOL_CPU
        assert (grads[k][~live] == 0).all()
    assert np.abs(grads["gm"][0]).max() > 0


def test_cpu_mode_with_lengths():
    lens = gc.RAGGED_LENGTHS
    want = gc.expected("main", tuple(lens))
    scores, grads = cpu_mode("main", lengths=lens)
    np.testing.assert_allclose(scores[:3, 0], want["scores"][:3, 0], rtol=0, atol=gc.ATOL_SCORE_CPU)
    np.testing.assert_allclose(scores[:3, 1:], want["scores"][:3, 1:], rtol=gc.ATOL_SCORE_CPU, atol=0)
    for k in gc.KEYS:
        assert gc.row_errors(grads[k], want[k]).max() <= gc.RTOL_CPU
        for b, n in enumerate(lens):
            assert (grads[k][b, n:] == 0).all()
        assert (grads[k][3] == 0).all()
    assert np.isnan(scores[3]).all() and np.abs(grads["gm"][1]).max() > 0


def test_the_float32_yardstick_and_the_bar():
    worst = max(float(v.max()) for v in gc.yardstick().values())
    print(f"float32 restatement against the float64 reference: worst row error {worst:.3e}; bar {gc.bar():.3e}")
    print({k: v.max(0).tolist() for k, v in gc.yardstick().items()})
    assert 1e-6 < worst < 5e-4 and gc.bar() == gc.BAR_FACTOR * worst   # (a wrong adjoint is off by 1e-2 or more)


def test_loss():
    m = PESQ(16000)
    c, d = gc.rows("main")
    lens = gc.RAGGED_LENGTHS
    want = gc.expected("main", tuple(lens))
    sc = want["scores"][:3]
    est = d.clone().requires_grad_(True)
    for key, value, ref in (("PESQ", -sc[:, 0].mean(), -want["gm"] / 3),
                            ("distance", (0.1 * sc[:, 1] + 0.0309 * sc[:, 2]).mean(),
                             (0.1 * want["gs"] + 0.0309 * want["ga"]) / 3)):
        est.grad = None
        loss = m.loss(c, est, lengths=lens, key=key)
        assert loss.dtype == torch.float64 and loss.dim() == 0
        assert abs(float(loss.detach()) - value) <= 1e-12
        loss.backward()
        assert est.grad.dtype == torch.float32 and (est.grad[3] == 0).all()
        np.testing.assert_allclose(est.grad.numpy(), ref.astype(np.float32), rtol=2.0 ** -22, atol=1e-12)
    assert float(m.loss(c, d).detach()) == float(m.loss(c, d, key="PESQ").detach())
    with pytest.raises(ValueError, match="key"):
        m.loss(c, d, key="MOS")
    # no scored row: a zero that carries a zero gradient
    short = d[:, :3000].clone().requires_grad_(True)
    loss = m.loss(c[:, :3000], short, lengths=[3000] * 4)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert (short.grad == 0).all() and short.grad.shape == short.shape
    with pytest.raises(RuntimeError, match="size is 20"):   # without lengths: as scores()
        m.loss(c[:, :3000], short)
    # other rates go through the float64 resampler in CPU mode
    c8, d8 = c[:2, ::2].contiguous(), d[:2, ::2].clone().requires_grad_(True)
    m8 = PESQ(8000)
    s8 = m8.differentiable_scores(c8, d8, 8000)
    np.testing.assert_allclose(s8.detach().numpy(), m8.scores(c8, d8.detach(), sample_rate=8000).numpy(), rtol=0, atol=1e-3)
    s8.sum().backward()
    assert bool(torch.isfinite(d8.grad).all()) and float(d8.grad.abs().max()) > 0
    half = d.to(torch.bfloat16).requires_grad_(True)
    m.loss(c, half).backward()
    assert half.grad.dtype == torch.bfloat16 and bool(torch.isfinite(half.grad.float()).all())


def test_refusals_and_detached_scores():
    m = PESQ(16000)
    c, d = gc.rows("main")
    src = c.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="constants"):
        m.differentiable_scores(src, d)
    with pytest.raises(NotImplementedError, match="constants"):
        m.loss(src, d.clone().requires_grad_(True))
    with torch.no_grad():
        assert m.differentiable_scores(src, d).shape == (4,)   # (no graph asked for)
    with pytest.raises(ValueError, match="sample_rate"):
        PESQ(8000).loss(c, d)   # an 8 kHz metric must be told its rows' rate
    for mode in (True, "row", "utterance", "p862"):
        with pytest.raises(NotImplementedError, match="time_align"):
            PESQ(16000, time_align=mode).loss(c, d)
        with pytest.raises(NotImplementedError, match="time_align"):
            PESQ(16000, time_align=mode).differentiable_scores(c, d)

    class Shards:   # (a fan-out needs GPUs to construct: stand in for one)
        pass

    fan = PESQ(16000)
    fan._fanout = Shards()
    with pytest.raises(NotImplementedError, match="devices"):
        fan.differentiable_scores(c, d)
    with pytest.raises(NotImplementedError, match="devices"):
        fan.loss(c, d)
    # scores() stays detached
    est = d.clone().requires_grad_(True)
    s = m.scores(c, est)
    assert s.grad_fn is None and not s.requires_grad
    assert not m.scores(src, est, lengths=gc.RAGGED_LENGTHS).requires_grad
