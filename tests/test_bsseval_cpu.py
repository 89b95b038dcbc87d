"""BSSEval without a GPU: the four C entries (declared, exported, bound; their refusals, answered on
the host before any launch), the package's CPU mode against the float64 statement of the definition
(tests/bsseval_cases.py), the literal s_target / e_interf / e_artif decomposition, the one-source
corner against BSSSDR and the reference's goldens, the assignment, SDRi, the NaN rule and the class
API."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import BSSEval, _build, _cpu, _native

from . import contract
from . import bsseval_cases as bc
from . import bsssdr_cases as sc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("fsem_bsseval_max_sources", "fsem_bsseval_corr_doubles", "fsem_bsseval_f32", "fsem_bsseval_scores_f32")


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.fixture(scope="module")
def metric():
    return BSSEval(16000)


def test_entries_are_declared_exported_and_bound(lib):
    contract.entries_are_declared_exported_and_bound(lib, "fsem_bsseval_", ENTRIES)
    assert "bsseval.hip" in _build.SOURCES


def test_queries(lib):
    assert lib.fsem_bsseval_max_sources() == 4 == BSSEval.MAX_SOURCES == _cpu.BSSEVAL_MAX_SOURCES
    # per mixture: (S^2 + S E) 512 summed lags, as many per 32768-sample chunk, S + E norm records per 8192
    for S, E, L in ((1, 1, 1), (2, 2, 160000), (4, 4, 32768), (2, 1, 32769), (3, 2, 1 << 29)):
        pairs, chunks, nchunks = S * S + S * E, -(-L // 32768), -(-L // 8192)
        assert lib.fsem_bsseval_corr_doubles(S, E, L) == pairs * 512 * (1 + chunks) + (S + E) * nchunks
    for S, E, L in ((0, 1, 100), (5, 1, 100), (1, 0, 100), (1, 5, 100), (2, 2, 0), (2, 2, (1 << 29) + 1)):
        assert lib.fsem_bsseval_corr_doubles(S, E, L) == 0


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(16), None
    big = (1 << 29) + 1
    EINVAL, OK = _native.FSEM_EINVAL, _native.FSEM_OK
    call = contract.by_name(lib.fsem_bsseval_f32, "src est batch S E length ld lengths norms corr coh coh_all", null)
    ok = dict(src=p, est=p, batch=3, S=2, E=2, length=8000, ld=8000, lengths=null, norms=p, corr=p, coh=p, coh_all=p)
    contract.refusals(call, ok, contract.nulled(EINVAL, "src est norms corr coh coh_all") + contract.each(
        EINVAL, dict(batch=-1), dict(S=0), dict(S=5), dict(E=0), dict(E=5), dict(length=0), dict(ld=7999),
        dict(length=big, ld=big)) + contract.each(OK, dict(batch=0)))  # nothing to score, nothing launched
    scores = contract.by_name(lib.fsem_bsseval_scores_f32, "coh coh_all batch S E crit sdr sir sar perm sdm sim", null)
    oks = dict(coh=p, coh_all=p, batch=3, S=2, E=2, crit=1, sdr=p, sir=p, sar=p, perm=p, sdm=null, sim=null)
    contract.refusals(scores, oks, contract.nulled(EINVAL, "coh coh_all sdr sir sar perm") + contract.each(
        EINVAL, dict(batch=-1), dict(S=0), dict(S=5), dict(E=0), dict(E=5), dict(crit=-1), dict(crit=3), dict(S=1, E=2))
        + contract.each(OK, dict(batch=0), dict(batch=0, sdm=p, sim=p)))


def test_cases_are_stable():
    """The two float64 evaluations of the definition agree on (nearly) every mixture of the tests."""
    keeps = [bc.case(*shape)[2]["keep"] for shape in bc.SHAPES] + [bc.ragged_batch()[3]["keep"]]
    keeps.append(bc.expected(*(x[None] for x in bc.near_source_mixture()))["keep"])
    keep = np.concatenate(keeps)
    print(f"{int((~keep).sum())} of {keep.size} mixtures dropped as unstable")
    assert (~keep).sum() * 8 <= keep.size


@pytest.mark.parametrize("shape", bc.SHAPES, ids=lambda s: "S%d-E%d-n%d" % s)
def test_cpu_mode_against_the_definition(metric, shape):
    s, h, want = bc.case(*shape)
    got = metric.scores(s, h, return_matrix=True)
    assert [g.dtype for g in got] == [torch.float32] * 3 + [torch.int32] + [torch.float32] * 2
    assert got[0].shape == (1, shape[1]) and got[4].shape == (1, shape[0], shape[1])
    bc.assert_all_close(got, want, f"cpu mode {shape}")


def test_cpu_mode_with_lengths(metric):
    s, h, lens, want = bc.ragged_batch()
    bc.assert_all_close(metric.scores(s, h, lengths=lens, return_matrix=True), want, "cpu mode, ragged batch")
    bc.assert_all_close(metric.scores(s, h, lengths=lens.tolist()), want, "cpu mode, lengths as a list")


def test_near_source_estimate_scores_beyond_60_db(metric):
    s, h = (x[None] for x in bc.near_source_mixture())
    want = bc.expected(s, h)
    assert want["keep"].all() and want["SDR"][0, 0] > sc.HIGH_DB and want["SIR"][0, 0] > sc.HIGH_DB
    bc.assert_all_close(metric.scores(s, h, return_matrix=True), want, "cpu mode, an estimate near its source")


def test_literal_decomposition():
    """s_target, e_interf and e_artif by least squares on the matrix of delayed sources (S = 2, n = 1100):
    their energy ratios are the three scores."""
    S, E, n = 2, 2, 1100
    s, h = bc.mixture(S, E, n)
    sn = np.stack([bc.normalise(r) for r in s.numpy()])
    hn = np.stack([bc.normalise(r) for r in h.numpy()])
    N = n + bc.K - 1
    delayed = np.zeros((S, bc.K, N))
    for i in range(S):
        for k in range(bc.K):
            delayed[i, k, k:k + n] = sn[i]
    A = delayed.reshape(S * bc.K, N).T
    want = bc.expected(s[None], h[None], criterion=None)
    for e in range(E):
        y = np.concatenate([hn[e], np.zeros(bc.K - 1)])
        p_all = A @ np.linalg.lstsq(A, y, rcond=None)[0]
        e_artif = y - p_all
        sar = 10 * np.log10(np.sum(p_all ** 2) / np.sum(e_artif ** 2))
        assert abs(sar - want["SAR"][0, e]) <= sc.ATOL_DB, (e, sar, want["SAR"][0, e])
        for i in range(S):
            Ai = A[:, i * bc.K:(i + 1) * bc.K]
            s_target = Ai @ np.linalg.lstsq(Ai, y, rcond=None)[0]
            e_interf = p_all - s_target
            sdr = 10 * np.log10(np.sum(s_target ** 2) / np.sum((e_interf + e_artif) ** 2))
            sir = 10 * np.log10(np.sum(s_target ** 2) / np.sum(e_interf ** 2))
            print(f"pair ({i}, {e}): SDR {sdr:.6f} / {want['SDR_mat'][0, i, e]:.6f}, SIR {sir:.6f} / "
                  f"{want['SIR_mat'][0, i, e]:.6f}, SAR {sar:.6f} / {want['SAR'][0, e]:.6f}")
            assert abs(sdr - want["SDR_mat"][0, i, e]) <= sc.ATOL_DB
            assert abs(sir - want["SIR_mat"][0, i, e]) <= sc.ATOL_DB


def test_one_source_is_bsssdr(metric):
    """S = E = 1 (2-D rows): SDR is BSSSDR's, SAR equals SDR, and SIR -- no interference, the denominator at
    its clamp -- is 80 + 10 log10(coh), beyond 60 dB."""
    c, n = sc.speech_rows(4, 8000)
    sdr, sir, sar, perm = metric.scores(c, n)
    assert sdr.shape == (4, 1) and not perm.any()
    want, keep = sc.expected(c, n)
    sc.assert_close(sdr[:, 0], want, keep, "S = E = 1 against BSSSDR's definition")
    sc.assert_close(sdr[:, 0], _cpu.bsssdr(c, n).double().numpy(), keep, "S = E = 1 against _cpu.bsssdr")
    np.testing.assert_array_equal(sar.numpy(), sdr.numpy())
    ex = bc.expected(c, n)
    bc.assert_close(sir, ex["SIR"], ex["keep"], "S = E = 1 SIR")
    assert (sir > sc.HIGH_DB).all() and (sir <= 80).all()
    names = ("bsssdr_16k", "bsssdr_8k", "bsssdr_white")
    bar = sc.golden_bar(*names)
    for name in names:
        c, n, sr, ref, has_ref, ref_ok = sc.golden(name)
        res = BSSEval(sr)(c, n)
        assert [tuple(r) for r in res] == [BSSEval.KEYS] * len(res)
        sc.assert_close(res, ref, ref_ok, f"cpu call vs reference {name}", atol=bar)


def test_permutation(metric):
    s, h, want = bc.case(3, 3, 6000)
    assert want["perm"][0].tolist() == [0, 1, 2]
    sdr_mat, sir_mat = want["SDR_mat"][0], want["SIR_mat"][0]
    for order in ([1, 0, 2], [1, 2, 0], [2, 0, 1]):  # swapped, rotated both ways
        hp = h[:, order]
        for crit in ("SIR", "SDR"):
            got = BSSEval(16000, permutation=crit).scores(s, hp, return_matrix=True)
            assert got[3][0].tolist() == order, (order, crit)
            e = np.arange(3)
            bc.assert_close(got[0], np.diag(sdr_mat)[order][None], None, f"SDR, estimates {order}, {crit}")
            bc.assert_close(got[1], np.diag(sir_mat)[order][None], None, f"SIR, estimates {order}, {crit}")
            bc.assert_close(got[2], want["SAR"][:, order], None, f"SAR, estimates {order}, {crit}")
            bc.assert_all_close(got, bc.expected(s, hp, criterion=crit), f"estimates {order}, {crit}")
        got = BSSEval(16000, permutation=None).scores(s, hp)
        assert got[3][0].tolist() == [0, 1, 2]
        bc.assert_close(got[0], sdr_mat[e, order][None], None, f"no permutation, estimates {order}")
    # E < S: the identity, whatever the criterion
    s2, h2, w2 = bc.case(2, 1, 33500)
    assert metric.scores(s2, h2)[3].tolist() == [[0]] and w2["perm"].tolist() == [[0]]
    # equal means keep the first assignment: two equal estimates
    s4, h4 = bc.mixture(2, 2, 6000)
    h4 = torch.stack([h4[0], h4[0]])
    for crit in ("SIR", "SDR"):
        got = BSSEval(16000, permutation=crit).scores(s4[None], h4[None])
        assert got[3][0].tolist() == [0, 1], crit
    # the scores' own tie rule on exactly symmetric energies, and a strict preference
    coh = torch.tensor([[[0.5, 0.5], [0.25, 0.25]], [[0.2, 0.6], [0.6, 0.2]]], dtype=torch.float64)
    coh_all = torch.tensor([[0.8, 0.8], [0.9, 0.9]], dtype=torch.float64)
    for crit in ("SIR", "SDR"):
        assert _cpu.bsseval_scores(coh, coh_all, crit)[3].tolist() == [[0, 1], [1, 0]]
    assert _cpu.bsseval_scores(coh, coh_all, None)[3].tolist() == [[0, 1], [0, 1]]
    with pytest.raises(ValueError):
        BSSEval(16000, permutation="SAR")


def test_sdri_by_its_definition(metric):
    s, h, want = bc.case(2, 2, 33500)
    hp = h[:, [1, 0]]
    mix = s.sum(1)
    sdr, sir, sar, perm, sdri = metric.scores(s, hp, mixture=mix)
    assert perm[0].tolist() == [1, 0] and sdri.shape == (1, 2) and sdri.dtype == torch.float32
    base = bc.expected(s, mix[:, None], criterion=None)["SDR_mat"][0, :, 0]  # SDR(i, mixture)
    bc.assert_close(sdri, (np.diag(want["SDR_mat"][0])[[1, 0]] - base[[1, 0]])[None], None, "SDRi")
    out = metric.scores(s, hp, mixture=mix, return_matrix=True)
    assert len(out) == 7 and torch.equal(out[6], sdri)


def test_nan_rule_per_mixture(metric):
    s0, h0 = bc.mixture(2, 2, 1100)
    s = torch.stack([s0, s0, s0]).clone()
    h = torch.stack([h0, h0, h0]).clone()
    base = metric.scores(s, h, return_matrix=True)
    assert all(torch.isfinite(t).all() for t in base)

    def only_nan(got, m, what):
        for g, b in zip(got, base):
            if g.dtype == torch.int32:
                assert g[m].tolist() == [0, 1], what
                continue
            assert torch.isnan(g[m]).all(), what
            keep = [x for x in range(3) if x != m]
            np.testing.assert_array_equal(g[keep].numpy(), b[keep].numpy(), err_msg=what)

    s1 = s.clone()
    s1[1, 1] = 0.0
    only_nan(metric.scores(s1, h, return_matrix=True), 1, "a silent source")
    h1 = h.clone()
    h1[2, 0, 77] = float("nan")
    only_nan(metric.scores(s, h1, return_matrix=True), 2, "a NaN sample in an estimate")
    s2 = s.clone()
    s2[0, 1, 1099] = float("inf")
    only_nan(metric.scores(s2, h, return_matrix=True), 0, "an inf sample in a source")
    # n + 511 < S 512: 512 samples carry two sources' delays no longer, 513 do
    only_nan(metric.scores(s, h, lengths=[1100, 512, 1100], return_matrix=True), 1, "n + 511 < S 512")
    assert torch.isfinite(metric.scores(s, h, lengths=[513, 1100, 1100])[0]).all()
    ex = bc.expected(s1, h)
    assert np.isnan(ex["SDR"][1]).all() and ex["keep"].all()
    assert np.isnan(bc.expected(s, h, [1100, 512, 1100])["SAR"][1]).all()
    assert torch.isnan(metric.scores(s[:, :, :0], h[:, :, :0])[0]).all()


def test_silent_estimate(metric):
    s, h = bc.mixture(2, 2, 1100)
    h = h.clone()
    h[1] = 0.0
    sdr, sir, sar, perm, sdm, sim = metric.scores(s[None], h[None], return_matrix=True)
    assert sdr[0, 1] == sir[0, 1] == sar[0, 1] == -80.0
    assert (sdm[0, :, 1] == -80.0).all() and (sim[0, :, 1] == -80.0).all()
    bc.assert_all_close((sdr, sir, sar, perm, sdm, sim), bc.expected(s[None], h[None]), "a silent estimate")


def test_class_api(metric):
    import fast_se_metrics
    import fast_speech_enhancement_metrics_amd as pkg
    assert pkg.BSSEval is BSSEval and "BSSEval" in pkg.__all__
    assert fast_se_metrics.__all__ == ["STOI", "PESQ"] and not hasattr(fast_se_metrics, "BSSEval")
    assert BSSEval.KEYS == ("SDR", "SIR", "SAR") and BSSEval.higher_is_better is True and metric.permutation == "SIR"
    s, h = bc.mixture(2, 2, 1100)
    with pytest.raises(NotImplementedError, match="lists"):
        metric([s], [h])
    with pytest.raises(NotImplementedError, match="lists"):
        metric.scores([s], [h])
    with pytest.raises(NotImplementedError, match="devices"):
        BSSEval(16000, devices=[0, 0])
    with pytest.raises(ValueError):
        metric.scores(s[None, :1], h[None])  # more estimates than sources
    with pytest.raises(ValueError):
        metric.scores(torch.zeros(1, 5, 2000), torch.zeros(1, 1, 2000))
    with pytest.raises(ValueError, match="sample_rate"):
        BSSEval(8000).scores(s[None], h[None])
    # the drop-in call: one dict per mixture, the means over its estimates
    sb, hb, lens, _ = bc.ragged_batch()
    res = metric(sb, hb, lengths=lens)
    sdr, sir, sar, _ = metric.scores(sb, hb, lengths=lens)
    assert [tuple(r) for r in res] == [BSSEval.KEYS] * 3
    for k, t in zip(BSSEval.KEYS, (sdr, sir, sar)):
        np.testing.assert_array_equal(np.array([r[k] for r in res], np.float32), t.mean(1).numpy())
    # 8 kHz rows are resampled row by row, each mixture's length with its rows
    m8 = BSSEval(8000)
    s8, h8 = bc.mixture(2, 2, 6000)
    s8 = torch.stack([s8, s8.flip(0)])
    h8 = torch.stack([h8, h8.flip(0)])
    lens8 = [6000, 3000]
    s16, l16 = m8._at_16k(s8, lens8, 8000)
    h16, _ = m8._at_16k(h8, lens8, 8000)
    assert s16.shape == (2, 2, 12000) and l16.tolist() == [12000, 6000]
    bc.assert_all_close(m8.scores(s8, h8, sample_rate=8000, lengths=lens8), bc.expected(s16, h16, l16), "8 kHz")
