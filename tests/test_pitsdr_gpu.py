"""PITSDR on the HIP engine (csrc/pitsdr.hip) against the float64 statement of the definition
(tests/pitsdr_cases.py): scores, assignment and gradients at two rates and five (S, E) shapes over the
chunk and float4 edges, row layouts and streams (bitwise), batch independence, ragged lengths, the gain
cases, non-finite mixtures, the grid.y limit, the loss and the CPU mode.

Gradients are checked where the definition promises a value: a pair whose SI-SDR lies beyond +-100 dB (only
its sign and magnitude are specified there, e.g. the collinear rows of a one-sample mixture) gets no incoming
SI-SDR gradient."""
import ctypes

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import PITSDR, _native

from . import pitsdr_cases as pc
from . import sdr_cases as sc
from .contract import assert_bitwise, on_side_stream

pytestmark = pytest.mark.gpu


def run(m, s, h, lengths=None, g=None):
    """((si, snr, perm, si_mat, snr_mat), grad): the engine's scores of device mixtures and the gradient of
    sum(g[0] * si_mat + g[1] * snr_mat) with respect to the estimates."""
    est = h.detach().requires_grad_(True)
    out = m.scores(s, est, lengths=lengths, return_matrix=True)
    assert all(o.is_cuda for o in out) and [o.dtype for o in out] == [torch.float32] * 2 + [torch.int32] + \
        [torch.float32] * 2
    if g is None:
        return tuple(o.detach() for o in out), None
    (out[3] * g[0].cuda() + out[4] * g[1].cuda()).sum().backward()
    assert est.grad.shape == h.shape and est.grad.dtype == torch.float32
    return tuple(o.detach() for o in out), est.grad


def in_domain(g_si, want):
    """The incoming SI-SDR gradient, zero on the pairs beyond +-100 dB."""
    ok = np.isfinite(want["SI_mat"]) & (np.abs(want["SI_mat"]) <= 100)
    return g_si * torch.as_tensor(ok, dtype=g_si.dtype)


def check(m, s, h, lengths=None, what="", criterion="SI-SDR", zero_mean=False, tie_ok=False, seed=7):
    """Scores, perm and gradients of host mixtures on the engine against the definition."""
    want = pc.expected(s, h, lengths=lengths, zero_mean=zero_mean, criterion=criterion, tie_ok=tie_ok)
    g_si, g_snr = pc.incoming(s.shape[0], s.shape[1], h.shape[1], seed)
    g_si = in_domain(g_si, want)
    got, grad = run(m, s.cuda(), h.cuda(), lengths, (g_si, g_snr))
    pc.assert_all_close(got, want, what)
    wgrad, bound = pc.expected_grad(s, h, g_si, g_snr, lengths=lengths, zero_mean=zero_mean)
    pc.assert_grad_close(grad, wgrad, bound, what)
    return got, grad


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 2), (4, 4), (4, 1)], ids=lambda s: "S%d-E%d" % s)
@pytest.mark.parametrize("sr", [8000, 16000])
def test_parity_over_chunk_and_vector_edges(sr, shape):
    S, E = shape
    C = _native.load().fsem_pitsdr_chunk(sr)
    lens = [1, 3, C - 1, C, C + 1, 2 * C + 5]
    order = [(e + 1) % S for e in range(E)] if S == E else None
    s, h = pc.mixtures(len(lens), S, E, 2 * C + 5, sr, seed=11 + S + E, order=order)
    m = PITSDR(sr, use_gpu=True)
    # (mixtures of one and three samples have no margin to pin an assignment with: they are scored as given)
    check(m, s[2:], h[2:], lens[2:], f"gpu {sr} {shape}")
    check(PITSDR(sr, use_gpu=True, permutation=None), s[:2], h[:2], lens[:2], f"gpu {sr} {shape} n = 1, 3",
          criterion=None)
    for b in (0, 1, 5):  # the unpadded mixture alone: its own capacity, n % 4 != 0
        n = lens[b]
        check(PITSDR(sr, use_gpu=True, permutation=None), s[b:b + 1, :, :n].contiguous(), h[b:b + 1, :, :n].contiguous(),
              None, f"gpu {sr} {shape} n = {n} alone", criterion=None)


@pytest.fixture(scope="module")
def ragged():
    """A ragged 2 x 2 batch on the host, its lengths and a metric: n % 4 != 0 beside n == L and n == 0."""
    L = 8200
    s, h = pc.mixtures(5, 2, 2, L, seed=17, order=[1, 0])
    return s, h, [L, 8195, 4097, 0, 5], PITSDR(16000, use_gpu=True)


def test_layouts_are_bitwise_equal(ragged):
    s, h, lens, m = ragged
    B, S, L = s.shape
    g = pc.incoming(B, S, S, 3)
    sg, hg = s.cuda(), h.cuda()
    base = run(m, sg, hg, lens, g)
    want = pc.expected(s, h, lengths=lens, tie_ok=True)
    pc.assert_all_close(base[0], want, "contiguous")

    def wide(x, cap, off):
        buf = torch.full((B, S, cap), float("nan"), device="cuda")
        buf[:, :, off:off + L] = x
        return buf[:, :, off:off + L]

    for what, cap, off in (("capacity with ld % 4 != 0", L + 3, 0), ("capacity with ld % 4 == 0", L + 4, 0),
                           ("storage offset of 4 bytes", L + 4, 1), ("storage offset of 8 bytes, odd capacity", L + 3, 2)):
        sv, hv = wide(sg, cap, off), wide(hg, cap, off)
        assert not sv.is_contiguous() and sv.data_ptr() % 16 == (4 * off) % 16
        got = run(m, sv, hv, lens, g)
        assert_bitwise(got[0], base[0], what)
        assert_bitwise([got[1]], [base[1]], what + ", gradient")
    got = on_side_stream(lambda: run(m, sg, hg, lens, g))
    assert_bitwise(got[0], base[0], "side stream")
    assert_bitwise([got[1]], [base[1]], "side stream, gradient")


def test_batch_independence(ragged):
    s, h, lens, m = ragged
    g = pc.incoming(5, 2, 2, 3)
    sg, hg = s.cuda(), h.cuda()
    got, grad = run(m, sg, hg, lens, g)
    n = lens[2]
    alone, galone = run(m, sg[2:3, :, :n].contiguous(), hg[2:3, :, :n].contiguous(), None, (g[0][2:3], g[1][2:3]))
    assert_bitwise([o[2:3] for o in got], alone, "mixture 2 alone")
    assert_bitwise([grad[2:3, :, :n]], [galone], "mixture 2 alone, gradient")


def test_ragged_lengths_and_the_gradient_tail(ragged):
    s, h, lens, m = ragged
    B, S, L = s.shape
    got, grad = check(m, s, h, lens, "gpu ragged", tie_ok=True)
    assert torch.isnan(got[0][3]).all() and got[2][3].tolist() == [0, 1]
    for b, n in enumerate(lens):
        assert (grad[b, :, n:] == 0).all() and (n == 0 or grad[b, :, :n].abs().max() > 0)
    # through the C entry, into a buffer pre-filled with NaN: every element is written
    lib = _native.load()
    p = ctypes.c_void_p
    sg, hg = s.cuda(), h.cuda()
    lg = torch.tensor(lens, dtype=torch.int32, device="cuda")
    want = pc.expected(s, h, lengths=lens, tie_ok=True)
    g_si, g_snr = pc.incoming(B, S, S, 7)
    g_si = in_domain(g_si, want).cuda()
    g_snr = g_snr.cuda()
    sums = torch.empty(B, lib.fsem_pitsdr_sums_doubles(S, S, L, 16000), dtype=torch.float64, device="cuda")
    si, snr = torch.empty(B, S, S, device="cuda"), torch.empty(B, S, S, device="cuda")
    perm = torch.empty(B, S, dtype=torch.int32, device="cuda")
    st = _native.stream_handle(sg.device)
    assert lib.fsem_pitsdr_f32(p(sg.data_ptr()), p(hg.data_ptr()), B, S, S, L, L, p(lg.data_ptr()), 16000, 0, 1,
                               p(sums.data_ptr()), p(si.data_ptr()), p(snr.data_ptr()), p(perm.data_ptr()), st) == 0
    for cap in (L, L + 3):  # the float4 stores and the scalar ones
        out = torch.full((B, S, cap), float("nan"), device="cuda")
        assert lib.fsem_pitsdr_grad_f32(p(sg.data_ptr()), p(hg.data_ptr()), B, S, S, L, L, p(lg.data_ptr()), 0,
                                        p(sums.data_ptr()), p(g_si.data_ptr()), p(g_snr.data_ptr()),
                                        p(out.data_ptr()), cap, st) == 0
        assert_bitwise([out[:, :, :L]], [grad], f"C entry, grad_ld = {cap}")
        assert torch.isnan(out[:, :, L:]).all()  # (and nothing past the row's `length` elements)
    assert_bitwise([si, snr, perm], got[3:5] + (got[2],), "C entry, forward")


def test_gain_cases():
    s, h = pc.gain_mixtures()
    want = pc.expected(s, h)
    assert abs(want["SI"][0, 0] - 60.018) < 1e-3 and abs(want["SI"][1, 0] - 80.022) < 1e-3
    assert abs(want["SNR"][2, 0] - 89.980) < 1e-3
    got, _ = run(PITSDR(16000, use_gpu=True), s.cuda(), h.cuda())
    pc.assert_all_close(got, want, "gpu gain cases")
    # the gradient where float64 autograd itself resolves it: the 60 dB row (at 80 and 90 dB the float64
    # residual sum h^2 - T carries 2 and 6 of the bound's 8 units by itself, CPU mode against the definition)
    check(PITSDR(16000, use_gpu=True), s[:1], h[:1], None, "gpu gain case 60 dB")


def test_zero_mean_on_dc_rows():
    s, h = pc.dc_mixtures(*pc.mixtures(2, 2, 2, 9000, seed=13, order=[1, 0]))
    check(PITSDR(16000, use_gpu=True, zero_mean=True), s, h, [9000, 8191], "gpu zero_mean", zero_mean=True)


def test_edge_mixtures():
    s, h = pc.edge_mixtures()
    got, _ = run(PITSDR(16000, use_gpu=True), s.cuda(), h.cuda())
    pc.assert_all_close(got, pc.expected(s, h, tie_ok=True), "gpu edge mixtures")


def test_nonfinite_mixture_is_nan_alone(ragged):
    s, h, _, m = ragged
    s, h = s[:3, :, :5000].contiguous(), h[:3, :, :5000].contiguous()
    g = pc.incoming(3, 2, 2, 5)
    base, gbase = run(m, s.cuda(), h.cuda(), None, g)
    for where in ("source", "estimate"):
        s2, h2 = s.clone(), h.clone()
        (s2 if where == "source" else h2)[1, 1, 4321] = float("nan") if where == "source" else float("inf")
        got, grad = run(m, s2.cuda(), h2.cuda(), None, g)
        for o in (got[0], got[1], got[3], got[4]):
            assert torch.isnan(o[1]).all(), where
        assert got[2][1].tolist() == [0, 1] and (grad[1] == 0).all(), where
        assert_bitwise([o[[0, 2]] for o in got], [o[[0, 2]] for o in base], f"beside a non-finite {where}")
        assert_bitwise([grad[[0, 2]]], [gbase[[0, 2]]], f"beside a non-finite {where}, gradient")


@pytest.mark.parametrize("S", [3, 4])
def test_assignment_recovers_a_known_permutation(S):
    order = [2, 0, 1] if S == 3 else [3, 0, 1, 2]
    s, h = pc.mixtures(2, S, S, 4000, seed=31 + S, order=order)
    sg, hg = s.cuda(), h.cuda()
    for crit in ("SI-SDR", "SNR"):
        want = pc.expected(s, h, criterion=crit)
        assert want["perm"].tolist() == [order] * 2
        got, _ = run(PITSDR(16000, use_gpu=True, permutation=crit), sg, hg)
        pc.assert_all_close(got, want, f"gpu assignment S = {S}, {crit}")
    got, _ = run(PITSDR(16000, use_gpu=True, permutation=None), sg, hg)
    assert got[2].tolist() == [list(range(S))] * 2
    pc.assert_all_close(got, pc.expected(s, h, criterion=None), f"gpu no assignment S = {S}")


def test_equal_means_keep_the_first_assignment():
    s, h = pc.mixtures(1, 2, 2, 4000, seed=37)
    h = torch.stack([h[:, 1], h[:, 1]], 1)
    for crit in ("SI-SDR", "SNR"):
        want = pc.expected(s, h, criterion=crit, tie_ok=True)
        assert want["margin"][0] == 0.0 and want["perm"][0].tolist() == [0, 1]
        got, _ = run(PITSDR(16000, use_gpu=True, permutation=crit), s.cuda(), h.cuda())
        pc.assert_all_close(got, want, f"gpu tie, {crit}")


def test_past_grid_limit():
    NB, K = 65537, 7
    s, h = pc.mixtures(K, 2, 2, 16, seed=23, order=[1, 0])
    want = pc.expected(s, h)  # (asserts the margin of all seven)
    m = PITSDR(16000, use_gpu=True)
    g = pc.incoming(K, 2, 2, 9)
    small, gsmall = run(m, s.cuda(), h.cuda(), None, g)
    src = torch.arange(NB) % K
    big, gbig = run(m, s[src].cuda(), h[src].cuda(), None, (g[0][src], g[1][src]))
    for b in (0, 40000, NB - 1):
        one = {k: v[b % K:b % K + 1] for k, v in want.items()}
        pc.assert_all_close([o[b:b + 1] for o in big], one, f"mixture {b} of {NB}")
    assert_bitwise(big, [o[src.cuda()] for o in small], "every mixture past the grid limit")
    assert_bitwise([gbig], [gsmall[src.cuda()]], "every gradient past the grid limit")


def test_loss_backward_twice():
    s, h = pc.mixtures(2, 2, 2, 8000, seed=43, order=[1, 0])
    m = PITSDR(16000, use_gpu=True)
    want = pc.expected(s, h)
    g = torch.zeros(2, 2, 2)
    for b in range(2):
        for e in range(2):
            g[b, want["perm"][b, e], e] = -0.25
    wgrad, bound = pc.expected_grad(s, h, g, torch.zeros_like(g))
    grads = []
    for _ in range(2):
        est = h.cuda().requires_grad_(True)
        loss = m.loss(s.cuda(), est)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and abs(float(loss.detach()) + want["SI"].mean()) <= \
            sc.ATOL_SDR
        loss.backward()
        grads.append(est.grad)
    pc.assert_grad_close(grads[0], wgrad, bound, "gpu loss")
    assert_bitwise([grads[1]], [grads[0]], "a second loss().backward()")
    with pytest.raises(NotImplementedError, match="sources"):
        m.loss(s.cuda().requires_grad_(True), h.cuda())
    res = m(s.cuda(), h.cuda().requires_grad_(True))  # the drop-in call leaves no graph
    si, snr, _ = m.scores(s.cuda(), h.cuda())
    np.testing.assert_array_equal(np.array([r["SI-SDR"] for r in res], np.float32), si.mean(1).cpu().numpy())


def test_si_sdri_and_cpu_mode_agree():
    s, h = pc.mixtures(3, 2, 2, 12000, seed=29, order=[1, 0])
    lens = [12000, 8193, 100]
    mix = s.sum(1)
    gpu = PITSDR(16000, use_gpu=True).scores(s.cuda(), h.cuda(), lengths=lens, mixture=mix.cuda(), return_matrix=True)
    cpu = PITSDR(16000).scores(s, h, lengths=lens, mixture=mix, return_matrix=True)
    assert torch.equal(gpu[2].cpu(), cpu[2])
    for k in (0, 1, 3, 4, 5):
        pc.assert_scores_close(gpu[k], cpu[k].double().numpy(), f"gpu vs cpu mode [{k}]")
    want = pc.expected(s, h, lengths=lens)
    base = pc.expected(s, mix[:, None], lengths=lens, criterion=None)["SI_mat"][:, :, 0]
    pc.assert_scores_close(gpu[5], want["SI"] - np.take_along_axis(base, want["perm"], 1), "gpu SI-SDRi")
