"""SDR metric (SI-SDR, SNR, segmental SNR) on the HIP engine (csrc/sdr.hip) against the float64
statement of the definitions (tests/sdr_cases.py): parity at five rates, chunk and frame edges,
row layouts, streams, non-finite rows, the grid.y limit, devices= and the CPU mode."""
import functools
import math

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SDR, _native

from . import sdr_cases as sc
from . import contract
from . import pair_metrics as pm

pytestmark = pytest.mark.gpu
assert_bitwise = functools.partial(contract.assert_bitwise, names=SDR.KEYS)


@pytest.fixture(scope="module")
def rows16():
    """The 16 kHz parity rows (host), their float64 scores and a metric."""
    c, n = sc.speech_rows(4, 48000, 16000, snr_high=40)
    return c, n, sc.expected(c, n, 16000), SDR(16000, use_gpu=True)


@pytest.mark.parametrize("sr,B,L", [(8000, 4, 24000), (22050, 4, 30000), (44100, 3, 50000), (48000, 3, 60000)])
def test_parity_rates(sr, B, L):
    c, n = sc.speech_rows(B, L, sr, snr_high=40)
    got = SDR(sr, use_gpu=True).scores(c.cuda(), n.cuda())
    assert all(g.is_cuda and g.dtype == torch.float32 and g.shape == (B,) for g in got)
    sc.assert_close(got, sc.expected(c, n, sr), f"gpu {sr}")


def test_parity_16k_and_int16_scale(rows16):
    c, n, want, m = rows16
    sc.assert_close(m.scores(c.cuda(), n.cuda()), want, "gpu 16000")
    cs, ns = c * 32768, n * 32768  # (exact: powers of two)
    sc.assert_close(m.scores(cs.cuda(), ns.cuda()), sc.expected(cs, ns, 16000), "gpu 16000 x32768")


def test_gain_cases(rows16):
    x, y = sc.gain_batch()
    sc.assert_close(rows16[3].scores(x.cuda(), y.cuda()), sc.expected(x, y, 16000), "gpu gain")


def test_zero_mean_dc_rows(rows16):
    c, n = rows16[0], rows16[1]
    cd, nd = sc.dc_rows(c, n)
    zm = SDR(16000, use_gpu=True, zero_mean=True)
    got = zm.scores(cd.cuda(), nd.cuda())
    sc.assert_close(got, sc.expected(cd, nd, 16000, zero_mean=True), "gpu zero_mean")
    free = sc.expected(c - c.mean(1, keepdim=True), n - n.mean(1, keepdim=True), 16000)
    np.testing.assert_allclose(got[0].cpu().numpy(), free[0], rtol=0, atol=sc.ATOL_SDR)
    off = rows16[3].scores(cd.cuda(), nd.cuda())
    assert_bitwise(got[1:], off[1:], "zero_mean leaves SNR / SegSNR")


@pytest.mark.parametrize("sr", [16000, 22050])
def test_chunk_and_frame_edges(sr):
    lib = _native.load()
    hop, win = sc.hop_win(sr)
    C = lib.fsem_sdr_chunk(sr)
    assert C % hop == 0 and hop == lib.fsem_sdr_hop(sr)
    cap = 2 * C + hop + 1
    lens = [0, 1, 3, win - 1, win, win + 1, win + hop - 1, win + hop,
            C - 1, C, C + 1, C + win - 1, C + win, 2 * C + hop + 1, cap]
    c, n = sc.speech_rows(len(lens), cap, sr, seed=17, snr_high=40)
    m = SDR(sr, use_gpu=True)
    cg, ng = c.cuda(), n.cuda()
    got = m.scores(cg, ng, lengths=lens)
    sc.assert_close(got, sc.expected(c, n, sr, lengths=lens), f"gpu edges {sr}")
    for b, k in enumerate(lens):
        assert lib.fsem_sdr_frames(k, sr) == ((k - win) // hop + 1 if k >= win else 0)
        if k == 0:
            continue  # (a batch needs a sample; the row's NaNs are checked above)
        alone = m.scores(cg[b:b + 1, :k], ng[b:b + 1, :k])
        assert_bitwise([g[b:b + 1] for g in got], alone, f"row {b} (n = {k}) alone")


def test_nonfinite_rows():
    pm.nonfinite_rows("SDR")


def test_edge_semantics(rows16):
    c, n = sc.edge_rows()
    si, snr, seg = (v.cpu().numpy() for v in rows16[3].scores(c.cuda(), n.cuda()))
    sc.assert_close((si, snr, seg), sc.expected(c, n, 16000), "gpu edge semantics")
    assert si[0] == math.inf and snr[0] == math.inf and seg[0] == 35.0
    assert math.isnan(si[1]) and snr[1] == -math.inf and seg[1] == -10.0
    assert math.isnan(si[2]) and abs(snr[2]) < 1e-6
    assert math.isnan(si[3]) and math.isnan(snr[3]) and seg[3] == -10.0
    hop, win = sc.hop_win(16000)
    lens = [0, 1, win - 1, win, win + hop - 1, win + hop]
    c, n = sc.speech_rows(len(lens), win + hop, 16000, seed=13)
    res = rows16[3]([c[b, :k].cuda() for b, k in enumerate(lens)], [n[b, :k].cuda() for b, k in enumerate(lens)])
    assert [list(r) for r in res] == [["SI-SDR", "SNR", "SegSNR"]] * len(lens)
    sc.assert_close(np.array([[r[k] for r in res] for k in SDR.KEYS]), sc.expected(c, n, 16000, lengths=lens),
                    "gpu short list")


def test_past_grid_limit():
    pm.past_grid_limit("SDR")


def test_cpu_mode_agrees():
    pm.cpu_mode_agrees("SDR")


def test_abi_refuses_before_launch():
    pm.refuses_before_launch("SDR")
