"""BSSSDR with gradients on the HIP engine (csrc/bsssdr_grad.hip) against the float64 statement of
tests/bsssdr_grad_cases.py: the forward bitwise ``scores()``, the gradient under BAR on every parity case, the
conventions, reproducibility and batch independence, row layouts, the C entries themselves, rows past the grid's
limit, and a short ascent."""
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import BSSSDR, _native
from fast_speech_enhancement_metrics_amd.base import resample_rows

from . import bsssdr_cases as bc
from . import bsssdr_grad_cases as gc
from . import contract
from . import lsd_cases as lc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def metric(sr: int = 16000, diag=None) -> BSSSDR:
    m = BSSSDR(sr, use_gpu=True)
    m.load_diag = diag
    return m


def engine(c, n, sr=16000, lens=None, g=None, diag=None):
    """(scores [B] float32, gradient [B, L] float32, both on the device) for the incoming gradient g (ones)."""
    est = n.cuda().requires_grad_(True)
    sdr = metric(sr, diag).differentiable_scores(c.cuda(), est, sr, lengths=None if lens is None else list(lens))
    assert sdr.is_cuda and sdr.dtype == torch.float32 and sdr.shape == (c.shape[0],)
    g = torch.ones(c.shape[0]) if g is None else g
    sdr.backward(g.to(sdr))
    assert est.grad.dtype == torch.float32 and est.grad.shape == n.shape
    return sdr.detach(), est.grad


@functools.lru_cache(maxsize=None)
def expected(name):
    """(scores, gradient) of the statement for a named case; for rows at another rate, at the float32 16 kHz rows
    the engine's resampler makes of them (the rows the score is taken at)."""
    c, n, sr, lens, diag = gc.rows(name)
    if sr == 16000:
        return gc.expected(name)
    c16, n16, lens16 = resample_rows(c.cuda(), n.cuda(), list(lens), sr, 16000)
    return gc.expected_for(c, n, sr, lens, diag, (c16.cpu(), n16.cpu(), lens16.cpu().tolist()))


@pytest.mark.parametrize("name", gc.PARITY)
def test_forward_is_scores_and_gradient_is_under_the_bar(name):
    c, n, sr, lens, diag = gc.rows(name)
    want_s, want_g = expected(name)
    sdr, grad = engine(c, n, sr, lens, diag=diag)
    lens_l = None if lens is None else list(lens)
    contract.assert_bitwise(sdr, metric(sr, diag).scores(c.cuda(), n.cuda(), sr, lengths=lens_l), f"{name}: forward")
    scored = np.isfinite(want_s)
    got_s = sdr.double().cpu().numpy()
    assert (np.isnan(got_s) == ~scored).all() and np.abs(got_s - want_s)[scored & (want_s < bc.HIGH_DB)].max() <= bc.ATOL_DB
    err = gc.row_errors(grad.cpu().numpy(), want_g)
    g = gc.incoming(c.shape[0])
    err_g = gc.row_errors(engine(c, n, sr, lens, g, diag)[1].cpu().numpy(), want_g * g.double().numpy()[:, None])
    print(f"gpu {name}: scores {' '.join(f'{v:.2f}' for v in want_s)} dB; row errors "
          f"{' '.join(f'{v:.2e}' for v in err)} (ones), worst {err_g.max():.2e} (random incoming); bar {gc.BAR:.2e}; "
          f"float32 autograd {' '.join(f'{v:.1e}' for v in gc.float32_autograd(name))}")
    if sr != 16000:   # what the host resampler's float32 rows would leave instead of the engine's
        host = gc.row_errors(gc.expected(name)[1], want_g)
        print(f"gpu {name}: the statement at the host resampler's rows against the engine resampler's: "
              f"{' '.join(f'{v:.2e}' for v in host)}")
    assert bool(torch.isfinite(grad).all())
    assert gc.BAR <= gc.BAR_LIMIT
    assert err.max() <= gc.BAR and err_g.max() <= gc.BAR
    if lens is not None:
        for b, k in enumerate(lens):
            assert bool((grad[b, k:] == 0).all())


def test_conventions():
    c, n, _, _, _ = gc.rows("speech")
    c, n = c[:, :4000].contiguous(), n[:, :4000].contiguous()
    base_s, base_g = engine(c, n)
    for where, value in (("estimate", float("nan")), ("clean", float("inf")), ("estimate", float("-inf"))):
        cb, nb = c.clone(), n.clone()
        (nb if where == "estimate" else cb)[1, 3000] = value
        sdr, grad = engine(cb, nb)
        assert bool(torch.isnan(sdr[1])) and bool((grad[1] == 0).all())
        contract.assert_bitwise(sdr[[0, 2, 3]], base_s[[0, 2, 3]], f"{value} in the {where}: scores")
        contract.assert_bitwise(grad[[0, 2, 3]], base_g[[0, 2, 3]], f"{value} in the {where}: gradient")
    # the loss over the finite rows alone, with its sign
    nb = n.clone()
    nb[1, 3000] = float("nan")
    est = nb.cuda().requires_grad_(True)
    loss = metric().loss(c.cuda(), est)
    assert abs(float(loss.detach()) + float(base_s[[0, 2, 3]].double().mean())) <= 1e-5 * abs(float(loss.detach()))
    loss.backward()
    assert bool((est.grad[1] == 0).all()) and bool(torch.isfinite(est.grad).all())
    assert gc.row_errors(est.grad[[0, 2, 3]].cpu().numpy(), -base_g[[0, 2, 3]].double().cpu().numpy() / 3).max() <= 1e-6
    # a silent estimate: -80 and exact zeros; a silent clean row: NaN and exact zeros; identical rows: finite; an
    # estimate whose norm sits below its clamp: the clamped-norm rule; the neighbours unchanged
    cb, nb = torch.cat([c, c[:1]]), torch.cat([n, n[:1]])
    nb[0], cb[1], nb[2] = 0.0, 0.0, c[2]
    nb[3] = n[3] * (1e-7 / float(n[3].double().norm()))
    sdr, grad = engine(cb, nb)
    contract.assert_bitwise(sdr, metric().scores(cb.cuda(), nb.cuda()), "convention rows: forward")
    assert float(sdr[0]) == -80.0 and bool((grad[0] == 0).all())
    assert bool(torch.isnan(sdr[1])) and bool((grad[1] == 0).all())
    # (coh is the sum of squares of float32 quotients, 1 up to 1e-7: +80 at or above 1 - 1e-8, else 70 dB and up)
    assert bc.HIGH_DB <= float(sdr[2]) <= 80.0 + 1e-5 and bool(torch.isfinite(grad[2]).all())
    print(f"identical rows: {float(sdr[2]):.2f} dB, max |g| {float(grad[2].abs().max()):.3e}")
    assert gc.quotients(cb[3].numpy(), nb[3].numpy())[3]
    s3, g3 = gc.expected_row(cb[3].numpy(), nb[3].numpy())
    err = gc.row_errors(grad[3:4].cpu().numpy(), g3[None])[0]
    print(f"norm below its clamp: {float(sdr[3]):.3f} dB (statement {s3:.3f}), row error {err:.2e}")
    assert abs(float(sdr[3]) - s3) <= bc.ATOL_DB and err <= gc.BAR
    contract.assert_bitwise((sdr[4:], grad[4:]), (base_s[:1], base_g[:1]), "the row beside them")
    # scale invariance on unclamped rows: sum_u g[u] h[u] = D (2 / nh) (y . h - coh h' . h) is zero but for the float32
    # rounding of the quotients (h = nh h' and h' . h' = 1 hold to 1e-7), which is part of the definition: the
    # statement's own sum reaches 1.1e-6 max|g| |h|_1 on the 33 dB row, above a bar of 2.7e-7.  So the engine's sum is
    # held to the statement's, within BAR max|g| |h|_1.
    for b in range(4):
        h = n[b].double().numpy()
        ref = float(gc.expected_row(c[b].numpy(), n[b].numpy())[1] @ h)
        dot = float(base_g[b].double().cpu().numpy() @ h)
        bound = gc.BAR * float(base_g[b].abs().max()) * float(np.abs(h).sum())
        print(f"row {b}: sum g h {dot:.3e}, the statement's {ref:.3e}, bound {bound:.3e}")
        assert abs(dot - ref) <= bound
    # rows of no samples
    est = n[:, :0].cuda().requires_grad_(True)
    sdr = metric().differentiable_scores(c[:, :0].cuda(), est)
    contract.assert_bitwise(sdr.detach(), metric().scores(c[:, :0].cuda(), n[:, :0].cuda()), "no samples")
    (sdr.nan_to_num().sum() + est.sum()).backward()
    assert est.grad.shape == (4, 0)


def test_reproducible_and_independent_of_the_batch():
    c, n, _, lens, _ = gc.rows("edges")
    g = gc.incoming(c.shape[0])
    sdr, grad = engine(c, n, lens=lens, g=g)
    sdr2, grad2 = contract.on_side_stream(lambda: engine(c, n, lens=lens, g=g))
    contract.assert_bitwise((sdr2, grad2), (sdr, grad), "a second run, on a side stream")
    for b, k in enumerate(lens):
        _, alone = engine(c[b:b + 1, :k], n[b:b + 1, :k], g=g[b:b + 1])
        contract.assert_bitwise(alone, grad[b:b + 1, :k], f"row {b} (n = {k}) alone and unpadded")
    # first, last, and in a batch of another size and padded length
    order = [14, 3, 7, 0]
    width = lens[14] + 5
    cp, npad = torch.full((4, width), float("nan")), torch.full((4, width), 1e30)
    for i, b in enumerate(order):
        cp[i, :lens[b]], npad[i, :lens[b]] = c[b, :lens[b]], n[b, :lens[b]]
    _, other = engine(cp, npad, lens=[lens[b] for b in order], g=g[order])
    for i, b in enumerate(order):
        contract.assert_bitwise(other[i:i + 1, :lens[b]], grad[b:b + 1, :lens[b]], f"row {b} at position {i}")


def test_past_the_grid_limit():
    NB = 65536 + 3
    c, n = lc.speech_rows(4, 64, seed=19)
    reps = -(-NB // 4)
    _, big = engine(c.repeat(reps, 1)[:NB].contiguous(), n.repeat(reps, 1)[:NB].contiguous())
    for b in (0, 65535, 65536, NB - 1):
        _, alone = engine(c[b % 4:b % 4 + 1], n[b % 4:b % 4 + 1])
        contract.assert_bitwise(big[b:b + 1], alone, f"row {b} of {NB}")
    want = np.stack([gc.expected_row(c[b].numpy(), n[b].numpy())[1] for b in range(4)])
    assert gc.row_errors(big[:4].cpu().numpy(), want).max() <= gc.BAR


def test_layouts():
    c, n, _, _, _ = gc.rows("speech")
    c, n = c[:, :4096], n[:, :4096]
    sdr, grad = engine(c, n)
    # slices of wider tensors at a 13-float offset with an odd row stride: 4-byte aligned rows, ld > L
    wc, wn = torch.full((4, 4096 + 14), 3.0).cuda(), torch.full((4, 4096 + 14), -2.0).cuda()
    wc[:, 13:13 + 4096] = c.cuda()
    wn[:, 13:13 + 4096] = n.cuda()
    est = wn.requires_grad_(True)
    got = metric().differentiable_scores(wc[:, 13:13 + 4096], est[:, 13:13 + 4096])
    got.sum().backward()
    contract.assert_bitwise((got.detach(), est.grad[:, 13:13 + 4096]), (sdr, grad), "4-byte aligned rows")
    assert bool((est.grad[:, :13] == 0).all()) and bool((est.grad[:, 13 + 4096:] == 0).all())
    # a non-contiguous view: every other sample of a wider tensor
    wide = torch.zeros(4, 8192).cuda()
    wide[:, ::2] = n.cuda()
    est = wide.requires_grad_(True)
    got = metric().differentiable_scores(c.cuda(), est[:, ::2])
    got.sum().backward()
    contract.assert_bitwise((got.detach(), est.grad[:, ::2]), (sdr, grad), "a strided view")
    assert bool((est.grad[:, 1::2] == 0).all())
    # an odd length against its zero-padded copy with lengths
    sdr_o, grad_o = engine(c[:, :4093], n[:, :4093])
    cp, npad = torch.zeros(4, 4200), torch.zeros(4, 4200)
    cp[:, :4093], npad[:, :4093] = c[:, :4093], n[:, :4093]
    sdr_p, grad_p = engine(cp, npad, lens=[4093] * 4)
    contract.assert_bitwise((sdr_p, grad_p[:, :4093]), (sdr_o, grad_o), "odd length, padded with lengths")
    assert bool((grad_p[:, 4093:] == 0).all())
    # bfloat16 estimates: the float32 gradient of the rounded rows, in the estimate's dtype
    half = n.to(torch.bfloat16).cuda().requires_grad_(True)
    metric().differentiable_scores(c.cuda(), half).sum().backward()
    assert half.grad.dtype == torch.bfloat16
    _, g32 = engine(c, n.to(torch.bfloat16).float())
    contract.assert_bitwise(half.grad.float(), g32.to(torch.bfloat16).float(), "bfloat16 estimate")


def test_c_entries_padding_and_state_reuse():
    lib = _native.load()
    c, n, _, _, _ = gc.rows("speech")
    L = 4097
    g_all = gc.incoming(4)
    want_s, want = engine(c[:, :L], n[:, :L], g=g_all)
    stream = _native.stream_handle(torch.device("cuda"))
    # one state buffer, sized for the larger batch, serves two different batches in turn
    state = torch.empty(lib.fsem_bsssdr_state_floats(4, L), dtype=torch.float32, device="cuda")
    for rows_, ld, grad_ld in (([0, 1, 2, 3], 4100, 4104), ([2, 0], 4099, 4101), ([0, 1, 2, 3], 4099, 4098)):
        B = len(rows_)
        assert lib.fsem_bsssdr_state_floats(B, L) <= state.numel()
        cw, nw = torch.full((B, ld), float("nan")).cuda(), torch.full((B, ld), 1e30).cuda()
        cw[:, :L], nw[:, :L] = c[rows_, :L].cuda(), n[rows_, :L].cuda()
        g = g_all[rows_].cuda()
        sdr = torch.empty(B, device="cuda")
        rc = lib.fsem_bsssdr_state_f32(cw.data_ptr(), nw.data_ptr(), B, L, ld, None, 0.0, sdr.data_ptr(),
                                       state.data_ptr(), stream)
        assert rc == 0
        contract.assert_bitwise(sdr, want_s[rows_], f"rows {rows_}, ld {ld}: scores")
        outs = []
        for _ in range(2):   # (the backward leaves the state as it found it)
            grad = torch.full((B, grad_ld), 7.0, device="cuda")
            rc = lib.fsem_bsssdr_grad_f32(cw.data_ptr(), nw.data_ptr(), B, L, ld, None, g.data_ptr(), state.data_ptr(),
                                          grad.data_ptr(), grad_ld, stream)
            assert rc == 0
            assert bool((grad[:, L:] == 7.0).all())
            outs.append(grad[:, :L].clone())
        contract.assert_bitwise(outs[1], outs[0], f"rows {rows_}: the backward again")
        contract.assert_bitwise(outs[0], want[rows_], f"rows {rows_}, ld {ld}, grad_ld {grad_ld}")


def test_it_trains():
    """30 steps of gradient ascent (bsssdr_grad_cases.ascent) raise the SDR of one 4000-sample row at every step
    and by at least 3 dB; the step was chosen in CPU mode, where they take it from 5.67 to 11.90 dB."""
    first, trace = gc.ascent(metric(), "cuda")
    print(f"SDR {first:.3f} -> {' '.join(f'{v:.3f}' for v in trace)}")
    assert all(b > a for a, b in zip([first] + trace, trace)) and trace[-1] >= first + 3.0
