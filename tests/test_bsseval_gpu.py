"""BSSEval on the HIP engine (csrc/bsseval.hip) against the float64 statement of the definition
(tests/bsseval_cases.py): parity on the cases and a ragged batch, the correlation stage alone, the
resampler, the one-source corner against the BSSSDR engine and the reference's goldens, bitwise
invariance, lengths on each side of the kernels' edges, the NaN rule, the +-80 dB edges, the
assignment and the matrices against the CPU mode, and the drop-in call."""
import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import BSSSDR, BSSEval, _cpu, _native

from . import bsseval_cases as bc
from . import bsssdr_cases as sc
from .contract import assert_bitwise, on_side_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def metric():
    return BSSEval(16000, use_gpu=True)


@pytest.mark.parametrize("shape", bc.SHAPES, ids=lambda s: "S%d-E%d-n%d" % s)
def test_parity_on_the_cases(metric, shape):
    s, h, want = bc.case(*shape)
    got = metric.scores(s.cuda(), h.cuda(), return_matrix=True)
    assert all(g.is_cuda for g in got)
    assert [g.dtype for g in got] == [torch.float32] * 3 + [torch.int32] + [torch.float32] * 2
    bc.assert_all_close(got, want, f"gpu {shape}")


def test_parity_on_a_ragged_batch(metric):
    s, h, lens, want = bc.ragged_batch()
    bc.assert_all_close(metric.scores(s.cuda(), h.cuda(), lengths=lens, return_matrix=True), want, "gpu ragged batch")
    bc.assert_all_close(metric.scores(s.cuda(), h.cuda(), lengths=lens.cuda()), want, "gpu, device lengths")


def test_near_source_estimate_scores_beyond_60_db(metric):
    s, h = (x[None] for x in bc.near_source_mixture())
    bc.assert_all_close(metric.scores(s.cuda(), h.cuda(), return_matrix=True), bc.expected(s, h), "gpu near a source")


def test_correlations_alone(metric):
    """The documented head of `corr` -- C_ij (i-major), then b_ie -- against float64 inner products; the
    norms against the float32 statement."""
    S, E, n = 3, 2, 6000  # (an odd number of window signals: one group of a single signal)
    s, _ = bc.mixture(3, 3, n)
    h = bc.mixture(3, 3, n)[1][:E]
    coh, coh_all, norms, corr = BSSEval.engine_energies(s.cuda().contiguous(), h.cuda().contiguous(), 1, S, E, n, n,
                                                        None)
    C, b = bc.correlations(s.numpy(), h.numpy())
    got = corr[0, :(S * S + S * E) * 512].cpu().numpy()
    err_c = np.abs(got[:S * S * 512].reshape(S, S, 512) - C).max()
    err_b = np.abs(got[S * S * 512:].reshape(S, E, 512) - b).max()
    print(f"correlations: worst |C - definition| = {err_c:.3e}, |b - definition| = {err_b:.3e}")
    # unit-norm rows: the products of float32 quotients are exact in double and every partial sum is
    # below 1 in magnitude, so each of the two sums of n terms is within n 2^-53 of the exact value
    assert err_c <= 2 * n * 2.0 ** -53 and err_b <= 2 * n * 2.0 ** -53
    want = [max(np.float32(np.sqrt(np.sum(r.astype(np.float64) ** 2))), np.float32(1e-6))
            for r in list(s.numpy()) + list(h.numpy())]
    # (the double sums of squares differ in their order: equal up to the rounding to float32)
    np.testing.assert_allclose(norms[0].cpu().numpy(), np.array(want, np.float32), rtol=2.0 ** -23, atol=0)


def test_8k_rows_through_the_resampler():
    m8 = BSSEval(8000, use_gpu=True)
    s8, h8 = bc.mixture(2, 2, 6000)
    s8 = torch.stack([s8, s8.flip(0)]).cuda()
    h8 = torch.stack([h8, h8.flip(0)]).cuda()
    lens8 = [6000, 3000]
    s16, l16 = m8._at_16k(s8, lens8, 8000)
    h16, _ = m8._at_16k(h8, lens8, 8000)
    assert s16.shape == (2, 2, 12000) and l16.tolist() == [12000, 6000]
    want = bc.expected(s16, h16, l16)
    bc.assert_all_close(m8.scores(s8, h8, sample_rate=8000, lengths=lens8), want, "gpu scores 8 kHz")
    res = m8(s8, h8, lengths=lens8)
    for k in BSSEval.KEYS:
        bc.assert_close(np.array([r[k] for r in res]), want[k].mean(1), want["keep"], f"gpu call 8 kHz {k}")


def test_one_source_is_the_bsssdr_engine(metric):
    c, n = sc.speech_rows(4, 8000)
    sdr, sir, sar, perm = metric.scores(c.cuda(), n.cuda())
    assert sdr.shape == (4, 1) and not perm.any()
    ref = BSSSDR(16000, use_gpu=True).scores(c.cuda(), n.cuda())
    want, keep = sc.expected(c, n)
    sc.assert_close(sdr[:, 0], want, keep, "S = E = 1 against BSSSDR's definition")
    sc.assert_close(sdr[:, 0], ref.double().cpu().numpy(), keep, "S = E = 1 against the BSSSDR engine")
    assert_bitwise([sar], [sdr], "SAR is SDR at S = 1")
    assert (sir > sc.HIGH_DB).all() and (sir <= 80).all()
    names = ("bsssdr_16k", "bsssdr_8k", "bsssdr_white")
    bar = sc.golden_bar(*names)
    for name in names:
        c, n, sr, ref, has_ref, ref_ok = sc.golden(name)
        m = metric if sr == 16000 else BSSEval(sr, use_gpu=True)
        sc.assert_close(m(c.cuda(), n.cuda()), ref, ref_ok, f"gpu call vs reference {name}", atol=bar)


def test_batch_position_and_stride_invariance(metric):
    s, h, lens, _ = bc.ragged_batch()
    sg, hg = s.cuda(), h.cuda()
    base = metric.scores(sg, hg, lengths=lens, return_matrix=True)
    n = int(lens[2])
    alone = metric.scores(sg[2:3, :, :n].contiguous(), hg[2:3, :, :n].contiguous(), return_matrix=True)
    assert_bitwise(alone, [t[2:3] for t in base], "a mixture alone")
    # as the last of 5, behind mixtures of other lengths
    order = [0, 1, 0, 1, 2]
    last = metric.scores(sg[order], hg[order], lengths=lens[order], return_matrix=True)
    assert_bitwise([t[4:5] for t in last], alone, "a mixture as the last of 5")
    # a wider row stride: rows of capacity n in buffers of stride n + 37 (no alignment)
    ld = n + 37
    ws, wh = torch.full((2, ld), 7.0, device="cuda"), torch.full((2, ld), -3.0, device="cuda")
    ws[:, :n], wh[:, :n] = sg[2, :, :n], hg[2, :, :n]
    coh, coh_all, _, _ = BSSEval.engine_energies(ws, wh, 1, 2, 2, n, ld, None)
    wide = BSSEval._from_energies(coh, coh_all, "SIR", True)
    assert_bitwise(wide, alone, "a wider row stride")
    again = on_side_stream(lambda: metric.scores(sg, hg, lengths=lens, return_matrix=True))
    assert_bitwise(again, base, "a side stream")


def test_lengths_on_each_side_of_the_kernels_edges(metric):
    """n around the correlation record (32768) and the LDS piece (2048); the tails hold other data."""
    cap = 32769
    s0, h0 = bc.mixture(2, 2, cap)
    lens = [32767, 32769, 2047, 2049]
    s, h = torch.stack([s0] * 4), torch.stack([h0] * 4)
    want = bc.expected(s, h, lens)
    assert want["keep"].all()
    sp, hp = s.clone(), h.clone()
    for b, k in enumerate(lens):
        sp[b, :, k:] = float("nan")
        hp[b, :, k:] = 1e30
    bc.assert_all_close(metric.scores(sp.cuda(), hp.cuda(), lengths=lens, return_matrix=True), want, "gpu edges")


def test_nan_rule_and_the_80_db_edges(metric):
    s0, h0 = bc.mixture(2, 2, 1100)
    s = torch.stack([s0, s0, s0]).clone()
    h = torch.stack([h0, h0, h0]).clone()
    base = metric.scores(s.cuda(), h.cuda(), return_matrix=True)
    assert all(torch.isfinite(t).all() for t in base)

    def only_nan(got, m, what):
        keep = [x for x in range(3) if x != m]
        for g, b in zip(got, base):
            if g.dtype == torch.int32:
                assert g[m].tolist() == [0, 1], what
            else:
                assert torch.isnan(g[m]).all(), what
        assert_bitwise([g[keep] for g in got], [b[keep] for b in base], what)

    s1 = s.clone()
    s1[1, 1] = 0.0
    only_nan(metric.scores(s1.cuda(), h.cuda(), return_matrix=True), 1, "a silent source")
    h1 = h.clone()
    h1[2, 0, 77] = float("nan")
    only_nan(metric.scores(s.cuda(), h1.cuda(), return_matrix=True), 2, "a NaN sample in an estimate")
    s2 = s.clone()
    s2[0, 1, 1099] = float("inf")
    only_nan(metric.scores(s2.cuda(), h.cuda(), return_matrix=True), 0, "an inf sample in a source")
    only_nan(metric.scores(s.cuda(), h.cuda(), lengths=[1100, 512, 1100], return_matrix=True), 1, "n + 511 < S 512")
    assert torch.isfinite(metric.scores(s.cuda(), h.cuda(), lengths=[513, 1100, 1100])[0]).all()
    assert torch.isnan(metric.scores(s[:, :, :0].cuda(), h[:, :, :0].cuda())[0]).all()
    # a silent estimate: -80 / -80 / -80; an estimate equal to its source: beyond +60
    h3 = h0.clone()
    h3[1] = 0.0
    h3[0] = s0[0]
    got = metric.scores(s0[None].cuda(), h3[None].cuda(), return_matrix=True)
    sdr, sir, sar = (t.cpu() for t in got[:3])
    assert sdr[0, 1] == sir[0, 1] == sar[0, 1] == -80.0
    assert sdr[0, 0] >= sc.HIGH_DB and sir[0, 0] >= sc.HIGH_DB and sar[0, 0] >= sc.HIGH_DB and sdr.max() <= 80.001
    bc.assert_all_close(got, bc.expected(s0[None], h3[None]), "gpu +-80 dB edges")


def test_permutation_and_matrices_equal_the_cpu_modes():
    s, h, _ = bc.case(3, 3, 6000)
    s4, h4 = bc.mixture(2, 2, 6000)
    for crit in ("SIR", "SDR", None):
        gpu, cpu = BSSEval(16000, use_gpu=True, permutation=crit), BSSEval(16000, permutation=crit)
        for order in ([0, 1, 2], [1, 0, 2], [1, 2, 0], [2, 0, 1]):
            hp = h[:, order]
            g, c = gpu.scores(s.cuda(), hp.cuda(), return_matrix=True), cpu.scores(s, hp, return_matrix=True)
            assert g[3].cpu().tolist() == c[3].tolist() == ([order] if crit else [[0, 1, 2]])
            for a, b, name in zip(g, c, ("SDR", "SIR", "SAR", "perm", "SDR matrix", "SIR matrix")):
                if name != "perm":
                    bc.assert_close(a, b.double().numpy(), None, f"gpu vs cpu mode, {crit}, {order}, {name}")
        # equal means keep the first assignment: two equal estimates
        he = torch.stack([h4[0], h4[0]])
        assert gpu.scores(s4[None].cuda(), he[None].cuda())[3].cpu().tolist() == [[0, 1]]
    # the scores entry's own tie rule on exactly symmetric energies, and a strict preference
    coh = torch.tensor([[[0.5, 0.5], [0.25, 0.25]], [[0.2, 0.6], [0.6, 0.2]]], dtype=torch.float64)
    coh_all = torch.tensor([[0.8, 0.8], [0.9, 0.9]], dtype=torch.float64)
    for crit in ("SIR", "SDR", None):
        g = BSSEval._from_energies(coh.cuda(), coh_all.cuda(), crit, True)
        c = _cpu.bsseval_scores(coh, coh_all, crit)
        assert g[3].cpu().tolist() == c[3].tolist() == ([[0, 1], [1, 0]] if crit else [[0, 1], [0, 1]])
        for a, b in zip(g, c):
            np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=0, atol=1e-5)
    # E < S: the identity
    s2, h2, w2 = bc.case(2, 1, 33500)
    assert BSSEval(16000, use_gpu=True).scores(s2.cuda(), h2.cuda())[3].cpu().tolist() == [[0]]


def test_sdri_and_the_drop_in_call(metric):
    s, h, lens, want = bc.ragged_batch()
    sg, hg = s.cuda(), h.cuda()
    res = metric(sg, hg, lengths=lens)
    sdr, sir, sar, perm = metric.scores(sg, hg, lengths=lens)
    assert [tuple(r) for r in res] == [BSSEval.KEYS] * 3
    for k, t in zip(BSSEval.KEYS, (sdr, sir, sar)):
        np.testing.assert_array_equal(np.array([r[k] for r in res], np.float32), t.mean(1).cpu().numpy())
    mix = s.sum(1)
    out = metric.scores(sg, hg, lengths=lens, mixture=mix.cuda())
    base = bc.expected(s, mix[:, None], lens, criterion=None)["SDR_mat"][:, :, 0]  # SDR(i, mixture) [B, S]
    p = want["perm"].astype(np.int64)
    bc.assert_close(out[4], want["SDR"] - np.take_along_axis(base, p, 1), want["keep"], "gpu SDRi")
    cpu = BSSEval(16000).scores(s, h, lengths=lens, mixture=mix)
    bc.assert_close(out[4], cpu[4].double().numpy(), want["keep"], "gpu SDRi vs cpu mode")


def test_abi_refuses_before_launch(metric):
    lib = _native.load()
    x = torch.zeros(2, 2, 1000, device="cuda")
    coh = torch.zeros(2, 2, 2, dtype=torch.float64, device="cuda")
    ca = torch.zeros(2, 2, dtype=torch.float64, device="cuda")
    nrm = torch.zeros(2, 4, device="cuda")
    corr = torch.zeros(2, lib.fsem_bsseval_corr_doubles(2, 2, 1000), dtype=torch.float64, device="cuda")
    for S, E, L, ld in ((5, 2, 1000, 1000), (2, 0, 1000, 1000), (2, 2, 1000, 999), (2, 2, 0, 1000)):
        assert lib.fsem_bsseval_f32(x.data_ptr(), x.data_ptr(), 2, S, E, L, ld, None, nrm.data_ptr(), corr.data_ptr(),
                                    coh.data_ptr(), ca.data_ptr(), None) == _native.FSEM_EINVAL
    torch.cuda.synchronize()
    assert not corr.any() and not nrm.any()  # (nothing ran)
