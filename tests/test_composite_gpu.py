"""Composite metric (CSIG, CBAK, COVL with PESQ, LLR, WSS, SegSNR) on the HIP engine
(csrc/composite.hip) against the float64 statement of the definitions (tests/composite_cases.py):
parity at both rates, frame and chunk edges, long rows through the radix select, silent clean
frames, row layouts, streams, non-finite rows, devices= and the CPU mode."""
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import PESQ, Composite, _native

from . import composite_cases as cc
from . import sdr_cases as sc
from . import contract
from . import pair_metrics as pm

pytestmark = pytest.mark.gpu
assert_bitwise = functools.partial(contract.assert_bitwise, names=Composite.KEYS)


def assert_pesq_is_the_class(got, c, n, sr, lengths=None, what=""):
    """The PESQ key is what PESQ(sr, use_gpu=True).scores gives for the same rows and lengths."""
    want = PESQ(sr, use_gpu=True).scores(c, n, lengths, sample_rate=sr)
    np.testing.assert_array_equal(got[3].cpu().numpy(), want.cpu().numpy(), err_msg=f"{what} PESQ key")  # (NaN == NaN)


@pytest.fixture(scope="module", params=[8000, 16000])
def rows(request):
    """The parity rows of one rate (host), their float64 LLR / WSS and a metric."""
    sr = request.param
    c, n = cc.parity_rows(sr)
    return sr, c, n, cc.expected_llr_wss(c, n, sr), Composite(sr, use_gpu=True)


def test_parity_and_int16_scale(rows):
    sr, c, n, want, m = rows
    cg, ng = c.cuda(), n.cuda()
    got = m.scores(cg, ng)
    assert len(got) == 7 and all(g.is_cuda and g.dtype == torch.float32 and g.shape == (4,) for g in got)
    cc.assert_scores(got, c, n, sr, what=f"gpu {sr}", want=want)
    assert np.isfinite(cc.to_np(got)).all()
    assert_pesq_is_the_class(got, cg, ng, sr, what=f"gpu {sr}")
    cs, ns = c * 32768, n * 32768  # (exact: powers of two)
    got = m.scores(cs.cuda(), ns.cuda())
    cc.assert_scores(got, cs, ns, sr, what=f"gpu {sr} x32768")
    assert_pesq_is_the_class(got, cs.cuda(), ns.cuda(), sr, what=f"gpu {sr} x32768")


def test_frame_and_chunk_edges(rows):
    sr, m = rows[0], rows[4]
    lib = _native.load_composite()
    hop, win = sc.hop_win(sr)
    C = lib.fsem_composite_chunk(sr)
    assert C == 16 * hop
    c, n, lens = cc.edge_rows(sr, C)
    cg, ng = c.cuda(), n.cuda()
    got = m.scores(cg, ng, lengths=lens)
    cc.assert_scores(got, c, n, sr, lengths=lens, what=f"gpu edges {sr}", atol_llr=cc.ATOL_LLR_EDGE,
                     atol_wss=cc.ATOL_WSS_EDGE)
    assert_pesq_is_the_class(got, cg, ng, sr, lengths=lens, what=f"gpu edges {sr}")
    for b, k in enumerate(lens):
        if k == 0:
            continue  # (a batch needs a sample; the row's NaNs are checked above)
        kc = max(k, 5376 * sr // 16000)  # (a capacity PESQ's whole-batch form takes as well)
        alone = m.scores(cg[b:b + 1, :kc], ng[b:b + 1, :kc], lengths=[k])
        assert_bitwise([g[b:b + 1] for g in got], alone, f"row {b} (n = {k}) alone")


def test_long_row_through_the_select(rows):
    """A row of about 8000 frames (the row means' radix select has no length limit): 40 hops of
    speech repeated, so the frame values repeat with period 40 and the float64 side stays small;
    the repeats are exact ties at the K-th value."""
    sr, m = rows[0], rows[4]
    hop, win = sc.hop_win(sr)
    period, reps = 40, 200
    c, n = sc.speech_rows(1, period * hop, sr, seed=29, snr_high=20)
    cl, nl = c.repeat(1, reps), n.repeat(1, reps)
    F = (cl.shape[1] - win) // hop + 1
    assert F == period * reps - 3
    llr, wss = cc.frame_values(cl[0, :period * hop + win - hop].numpy(), nl[0, :period * hop + win - hop].numpy(), sr)
    assert len(llr) == period
    idx = np.arange(F) % period
    want = np.array([[cc.trimmed_mean(llr[idx])], [cc.trimmed_mean(wss[idx])]])
    got = m.scores(cl.cuda(), nl.cuda())
    g = cc.to_np(got)
    for name, k, atol in (("LLR", 4, cc.ATOL_LLR), ("WSS", 5, cc.ATOL_WSS)):
        err = abs(g[k, 0] - want[k - 4, 0])
        print(f"gpu long row {sr} {name}: |got - float64 definition| = {err:.3e} over {F} frames")
        assert err <= atol, (name, g[k, 0], want[k - 4, 0])
    cc.assert_composites(g, f"gpu long row {sr}")
    assert np.isfinite(g).all()


@pytest.mark.parametrize("zeroed_ms", [75, 187.5])
def test_silent_clean_head(rows, zeroed_ms):
    """Digitally silent clean frames: NaN LLR frames (NaN row LLR once more than F - K of them), and
    clean band energies that sit exactly on the 1e-10 floor (WSS within its bar)."""
    sr, m = rows[0], rows[4]
    c, n = cc.silent_head_rows(sr, int(zeroed_ms * sr / 1000))
    want = cc.expected_llr_wss(c, n, sr)
    assert np.isnan(want[0, 0]) == (zeroed_ms > 100) and np.isfinite(want[1, 0])
    got = m.scores(c.cuda(), n.cuda())
    cc.assert_scores(got, c, n, sr, what=f"gpu silent head {sr} {zeroed_ms} ms", want=want)


def test_nonfinite_rows(rows):
    pm.nonfinite_rows(f"Composite-{rows[0]}")


def test_cpu_mode_agrees(rows):
    pm.cpu_mode_agrees(f"Composite-{rows[0]}")


def test_abi_refuses_before_launch():
    pm.refuses_before_launch("Composite")
