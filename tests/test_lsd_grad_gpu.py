"""LSD with gradients on the HIP engine (csrc/lsd_grad.hip, the transposed resampler of csrc/resample.hip)
against the float64 statement of tests/lsd_grad_cases.py: the forward bitwise ``scores()``, the gradient under
BAR on every parity case, the conventions, reproducibility and batch independence, row layouts, the C entries
themselves, the same for the other-rate backward (fsem_lsd_grad_rate_f32) at 8 and 48 kHz, and a short descent."""
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import LSD, _cpu, _native

from . import contract
from . import lsd_cases as lc
from . import lsd_grad_cases as gc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def metric(sr: int = 16000) -> LSD:
    return LSD(sr, use_gpu=True)


def engine(c, n, sr=16000, lens=None, g=None):
    """(scores [B] float32, gradient [B, L] float32, both on the device) for the incoming gradient g (ones)."""
    est = n.cuda().requires_grad_(True)
    lsd = metric(sr).differentiable_scores(c.cuda(), est, sr, lengths=None if lens is None else list(lens))
    assert lsd.is_cuda and lsd.dtype == torch.float32 and lsd.shape == (c.shape[0],)
    g = torch.ones(c.shape[0]) if g is None else g
    lsd.backward(g.to(lsd))
    assert est.grad.dtype == torch.float32 and est.grad.shape == n.shape
    return lsd.detach(), est.grad


@pytest.mark.parametrize("name", gc.PARITY)
def test_forward_is_scores_and_gradient_is_under_the_bar(name):
    c, n, sr, lens = gc.rows(name)
    want_s, want_g = gc.expected(name)
    lsd, grad = engine(c, n, sr, lens)
    lens_l = None if lens is None else list(lens)
    contract.assert_bitwise(lsd, metric(sr).scores(c.cuda(), n.cuda(), sr, lengths=lens_l), f"{name}: forward")
    if sr == 16000:   # (other rates: scores() on the engine's own float32-resampled rows, tests/test_lsd_gpu.py)
        lc.assert_close(lsd, want_s, f"gpu {name}")
    err = gc.row_errors(grad.cpu().numpy(), want_g)
    g = gc.incoming(c.shape[0])
    err_g = gc.row_errors(engine(c, n, sr, lens, g)[1].cpu().numpy(), want_g * g.double().numpy()[:, None])
    print(f"gpu {name}: row errors {' '.join(f'{v:.2e}' for v in err)} (ones), worst {err_g.max():.2e} (random "
          f"incoming); bar {gc.BAR:.2e}; float32 autograd {' '.join(f'{v:.1e}' for v in gc.float32_autograd(name))}")
    assert bool(torch.isfinite(grad).all())
    assert gc.BAR <= gc.BAR_LIMIT
    assert err.max() <= gc.BAR and err_g.max() <= gc.BAR
    if lens is not None:
        for b, k in enumerate(lens):
            assert bool((grad[b, k:] == 0).all())


def test_conventions():
    c, n, _, _ = gc.rows("speech")
    base_s, base_g = engine(c, n)
    for where, value in (("estimate", float("nan")), ("clean", float("inf")), ("estimate", float("-inf"))):
        cb, nb = c.clone(), n.clone()
        (nb if where == "estimate" else cb)[1, 5000] = value
        lsd, grad = engine(cb, nb)
        assert bool(torch.isnan(lsd[1])) and bool((grad[1] == 0).all())
        contract.assert_bitwise(lsd[[0, 2, 3]], base_s[[0, 2, 3]], f"{value} in the {where}: scores")
        contract.assert_bitwise(grad[[0, 2, 3]], base_g[[0, 2, 3]], f"{value} in the {where}: gradient")
    # the loss over the finite rows alone
    nb = n.clone()
    nb[1, 5000] = float("nan")
    est = nb.cuda().requires_grad_(True)
    loss = metric().loss(c.cuda(), est)
    assert abs(float(loss.detach()) - float(base_s[[0, 2, 3]].double().mean())) <= 1e-6 * float(loss.detach())
    loss.backward()
    assert bool((est.grad[1] == 0).all()) and bool(torch.isfinite(est.grad).all())
    # silent clean, silent estimate, both silent: exact zeros; identical up to a gain: finite (a residual)
    ce, ne = lc.edge_rows()
    lsd, grad = engine(ce, ne)
    contract.assert_bitwise(lsd, metric().scores(ce.cuda(), ne.cuda()), "edge rows: forward")
    assert bool(torch.isfinite(grad).all()) and bool((grad[1:4] == 0).all())
    for b in (0, 4, 5):
        w = gc.expected_row(ce[b].numpy(), ne[b].numpy())[1]
        print(f"{lc.EDGE_NAMES[b]}: row error {gc.row_errors(grad[b:b + 1].cpu().numpy(), w[None])[0]:.2e} "
              f"(not under the bar: a residual of cancelling terms)")
    # a one-sample row in a padded batch: finite, zeros past it
    lsd, grad = engine(c[:, :64], n[:, :64], lens=[1, 64, 2, 63])
    assert bool(torch.isfinite(lsd).all()) and bool(torch.isfinite(grad).all())
    for b, k in enumerate([1, 64, 2, 63]):
        assert bool((grad[b, k:] == 0).all())
    # rows of no samples
    est = n[:, :0].cuda().requires_grad_(True)
    lsd = metric().differentiable_scores(c[:, :0].cuda(), est)
    contract.assert_bitwise(lsd.detach(), metric().scores(c[:, :0].cuda(), n[:, :0].cuda()), "no samples")
    lsd.sum().backward()
    assert est.grad.shape == (4, 0)


def test_reproducible_and_independent_of_the_batch():
    c, n, _, lens = gc.rows("edges")
    g = gc.incoming(c.shape[0])
    lsd, grad = engine(c, n, lens=lens, g=g)
    lsd2, grad2 = contract.on_side_stream(lambda: engine(c, n, lens=lens, g=g))
    contract.assert_bitwise((lsd2, grad2), (lsd, grad), "a second run, on a side stream")
    for b, k in enumerate(lens):
        _, alone = engine(c[b:b + 1, :k], n[b:b + 1, :k], g=g[b:b + 1])
        contract.assert_bitwise(alone, grad[b:b + 1, :k], f"row {b} (n = {k}) alone and unpadded")


def test_past_the_grid_limit():
    NB = 65536 + 3
    c, n = lc.speech_rows(4, 300, seed=19)
    reps = -(-NB // 4)
    _, big = engine(c.repeat(reps, 1)[:NB].contiguous(), n.repeat(reps, 1)[:NB].contiguous())
    for b in (0, 65535, 65536, NB - 1):
        _, alone = engine(c[b % 4:b % 4 + 1], n[b % 4:b % 4 + 1])
        contract.assert_bitwise(big[b:b + 1], alone, f"row {b} of {NB}")
    err = gc.row_errors(big[:4].cpu().numpy(), np.stack([gc.expected_row(c[b].numpy(), n[b].numpy())[1] for b in range(4)]))
    assert err.max() <= gc.BAR


def test_layouts():
    c, n, _, _ = gc.rows("speech")
    c, n = c[:, :4096], n[:, :4096]
    lsd, grad = engine(c, n)
    # slices of wider tensors at a 12-float offset with an odd row stride: the 4-byte load path
    wc, wn = torch.full((4, 4096 + 13), 3.0).cuda(), torch.full((4, 4096 + 13), -2.0).cuda()
    wc[:, 12:12 + 4096] = c.cuda()
    wn[:, 12:12 + 4096] = n.cuda()
    est = wn.requires_grad_(True)
    got = metric().differentiable_scores(wc[:, 12:12 + 4096], est[:, 12:12 + 4096])
    got.sum().backward()
    contract.assert_bitwise((got.detach(), est.grad[:, 12:12 + 4096]), (lsd, grad), "4-byte loads")
    assert bool((est.grad[:, :12] == 0).all()) and bool((est.grad[:, 12 + 4096:] == 0).all())
    # an odd length against its zero-padded copy with lengths
    lsd_o, grad_o = engine(c[:, :4093], n[:, :4093])
    cp, npad = torch.zeros(4, 4200), torch.zeros(4, 4200)
    cp[:, :4093], npad[:, :4093] = c[:, :4093], n[:, :4093]
    lsd_p, grad_p = engine(cp, npad, lens=[4093] * 4)
    contract.assert_bitwise((lsd_p, grad_p[:, :4093]), (lsd_o, grad_o), "odd length, padded with lengths")
    assert bool((grad_p[:, 4093:] == 0).all())
    # bfloat16 estimates: the float32 gradient of the rounded rows, in the estimate's dtype
    half = n.to(torch.bfloat16).cuda().requires_grad_(True)
    metric().differentiable_scores(c.cuda(), half).sum().backward()
    assert half.grad.dtype == torch.bfloat16
    _, g32 = engine(c, n.to(torch.bfloat16).float())
    contract.assert_bitwise(half.grad.float(), g32.to(torch.bfloat16).float(), "bfloat16 estimate")


def test_c_entry_padding_and_state_reuse():
    lib = _native.load()
    c, n, _, _ = gc.rows("speech")
    B, L = 4, 4097
    _, want = engine(c[:, :L], n[:, :L], g=gc.incoming(B))
    g = gc.incoming(B).cuda()
    for ld, grad_ld in ((4100, 4104), (4099, 4101)):   # 16-byte and 4-byte rows
        cw, nw = torch.full((B, ld), float("nan")).cuda(), torch.full((B, ld), 1e30).cuda()
        cw[:, :L], nw[:, :L] = c[:, :L].cuda(), n[:, :L].cuda()
        state = torch.empty(lib.fsem_lsd_grad_state_floats(B, L), dtype=torch.float32, device="cuda")
        outs = []
        for _ in range(2):   # (the state reused)
            grad = torch.full((B, grad_ld), 7.0, device="cuda")
            rc = lib.fsem_lsd_grad_f32(cw.data_ptr(), nw.data_ptr(), B, L, ld, None, g.data_ptr(), state.data_ptr(),
                                       grad.data_ptr(), grad_ld, _native.stream_handle(grad.device))
            assert rc == 0
            assert bool((grad[:, L:] == 7.0).all())
            outs.append(grad[:, :L].clone())
        contract.assert_bitwise(outs[1], outs[0], f"ld {ld}: the state reused")
        contract.assert_bitwise(outs[0], want, f"ld {ld}, grad_ld {grad_ld}")


@pytest.mark.parametrize("orig", [8000, 48000])
def test_transposed_resampler(orig):
    lib = _native.load()
    rows, n_in, lens = 3, 3000, [1, 999, 3000]
    n_out = int(lib.fsem_resample_length(n_in, orig, 16000))
    gen = torch.Generator().manual_seed(41 + orig)
    g = torch.randn(rows, n_out, generator=gen)
    want = np.zeros((rows, n_in))
    for r, k in enumerate(lens):
        x = torch.zeros(1, k, dtype=torch.float64, requires_grad=True)
        y = _cpu.resample64(x, orig, 16000)
        want[r, :k] = torch.autograd.grad(y, x, grad_outputs=g[r:r + 1, :y.shape[1]].double())[0][0].numpy()
    gd, ld = g.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    grad = torch.full((rows, n_in + 3), 7.0, device="cuda")
    rc = lib.fsem_resample_rows_grad_f32(gd.data_ptr(), rows, n_in, n_out, ld.data_ptr(), grad.data_ptr(), n_in + 3,
                                         orig, 16000, _native.stream_handle(grad.device))
    assert rc == 0
    err = gc.row_errors(grad[:, :n_in].cpu().numpy(), want)
    print(f"transposed resampler {orig} -> 16000: row errors {' '.join(f'{v:.2e}' for v in err)}; bar {gc.BAR_RESAMPLE:.2e}")
    assert gc.BAR_RESAMPLE <= gc.BAR_LIMIT and err.max() <= gc.BAR_RESAMPLE
    assert bool((grad[:, n_in:] == 7.0).all())
    for r, k in enumerate(lens):
        assert bool((grad[r, k:n_in] == 0).all())
    # whole rows (lengths NULL) are the rows of full length
    full = torch.empty(rows, n_in, device="cuda")
    assert lib.fsem_resample_rows_grad_f32(gd.data_ptr(), rows, n_in, n_out, None, full.data_ptr(), n_in, orig, 16000,
                                           _native.stream_handle(grad.device)) == 0
    contract.assert_bitwise(full[2:3], grad[2:3, :n_in], "lengths NULL")


RATES = (8000, 48000)


@pytest.mark.parametrize("sr", RATES)
def test_other_rates_lengths_batch_and_non_finite_rows(sr):
    c, n, lens = gc.rate_rows(sr)
    want_s, want_g = gc.expected_for(c, n, sr, lens)
    g = gc.incoming(4)
    lsd, grad = engine(c, n, sr, lens, g)
    contract.assert_bitwise(lsd, metric(sr).scores(c.cuda(), n.cuda(), sr, lengths=list(lens)), f"{sr}: forward")
    err = gc.row_errors(grad.cpu().numpy(), want_g * g.double().numpy()[:, None])
    print(f"gpu {sr} with lengths {lens}: row errors {' '.join(f'{v:.2e}' for v in err)}; bar {gc.BAR:.2e}")
    assert bool(torch.isfinite(grad).all()) and err[:3].max() <= gc.BAR   # (the one-sample row: finite)
    for b, k in enumerate(lens):
        assert bool((grad[b, k:] == 0).all())
        _, alone = engine(c[b:b + 1, :k], n[b:b + 1, :k], sr, g=g[b:b + 1])
        contract.assert_bitwise(alone, grad[b:b + 1, :k], f"{sr}: row {b} (n = {k}) alone and unpadded")
    again = contract.on_side_stream(lambda: engine(c, n, sr, lens, g))
    contract.assert_bitwise(again, (lsd, grad), f"{sr}: a second run, on a side stream")
    # a non-finite sample inside a row's length, in either operand: NaN and a zero row, in that row only
    cb, nb = c.clone(), n.clone()
    nb[1, 100] = float("nan")
    cb[2, 200] = float("inf")
    lsd_b, grad_b = engine(cb, nb, sr, lens, g)
    assert bool(torch.isnan(lsd_b[1:3]).all()) and bool((grad_b[1:3] == 0).all())
    contract.assert_bitwise((lsd_b[[0, 3]], grad_b[[0, 3]]), (lsd[[0, 3]], grad[[0, 3]]), f"{sr}: rows beside them")


@pytest.mark.parametrize("sr", RATES)
def test_other_rates_c_entry_padding_and_state_reuse(sr):
    lib = _native.load()
    c, n, lens = gc.rate_rows(sr)
    B, L = c.shape
    g = gc.incoming(B)
    _, want = engine(c, n, sr, lens, g)
    gd, ld_ = g.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    for ld, grad_ld in ((L + 4, L + 8), (L + 5, L + 3)):
        cw, nw = torch.full((B, ld), float("nan")).cuda(), torch.full((B, ld), 1e30).cuda()
        cw[:, :L], nw[:, :L] = c.cuda(), n.cuda()
        state = torch.empty(lib.fsem_lsd_grad_rate_state_floats(B, L, sr), dtype=torch.float32, device="cuda")
        outs = []
        for _ in range(2):   # (the state reused)
            grad = torch.full((B, grad_ld), 7.0, device="cuda")
            rc = lib.fsem_lsd_grad_rate_f32(cw.data_ptr(), nw.data_ptr(), B, L, ld, ld_.data_ptr(), sr, gd.data_ptr(),
                                            state.data_ptr(), grad.data_ptr(), grad_ld,
                                            _native.stream_handle(grad.device))
            assert rc == 0
            assert bool((grad[:, L:] == 7.0).all())
            outs.append(grad[:, :L].clone())
        contract.assert_bitwise(outs[1], outs[0], f"{sr}, ld {ld}: the state reused")
        contract.assert_bitwise(outs[0], want, f"{sr}, ld {ld}, grad_ld {grad_ld}")


def test_other_rates_past_the_grid_limit():
    NB = 65536 + 3
    c, n = lc.speech_rows(4, 150, seed=19, sr=8000)
    reps = -(-NB // 4)
    _, big = engine(c.repeat(reps, 1)[:NB].contiguous(), n.repeat(reps, 1)[:NB].contiguous(), 8000)
    for b in (0, 65535, 65536, NB - 1):
        _, alone = engine(c[b % 4:b % 4 + 1], n[b % 4:b % 4 + 1], 8000)
        contract.assert_bitwise(big[b:b + 1], alone, f"row {b} of {NB}")
    assert gc.row_errors(big[:4].cpu().numpy(), gc.expected_for(c, n, 8000)[1]).max() <= gc.BAR


def test_it_trains():
    """Five Adam steps of size 1e-3 on the estimate's samples lower LSD on every ``speech`` row.  The step was
    chosen in CPU mode, where the same five steps lower the four rows by 0.42, 0.59, 0.93 and 0.42 (from
    10.11, 6.12, 5.88 and 6.58; a step of 3e-3 already raises two of them)."""
    c, n, _, _ = gc.rows("speech")
    cg = c.cuda()
    est = n.cuda().requires_grad_(True)
    opt = torch.optim.Adam([est], lr=1e-3)
    m = metric()
    first = m.scores(cg, est.detach()).clone()
    for _ in range(5):
        opt.zero_grad()
        m.loss(cg, est).backward()
        opt.step()
    last = m.scores(cg, est.detach())
    print(f"LSD {first.tolist()} -> {last.tolist()}")
    assert bool((last < first).all())
