"""LSD metric on the HIP engine (csrc/lsd.hip) against the float64 statement of the definition
(tests/lsd_cases.py) and the reference's scores: parity, gain and edge rows, frame and chunk edges,
row layouts, streams, non-finite rows, the grid.y limit, devices= and the CPU mode."""
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import LSD, _native

from . import lsd_cases as lc
from . import contract
from . import pair_metrics as pm

pytestmark = pytest.mark.gpu
assert_bitwise = functools.partial(contract.assert_bitwise, names=LSD.KEYS)


@pytest.fixture(scope="module")
def rows16():
    """The 16 kHz parity rows (host), their float64 scores and a metric."""
    c, n = lc.speech_rows(4, 48000)
    return c, n, lc.expected(c, n), LSD(16000, use_gpu=True)


def test_parity_16k_and_int16_scale(rows16):
    c, n, want, m = rows16
    got = m.scores(c.cuda(), n.cuda())
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (4,)
    lc.assert_close(got, want, "gpu 16000")
    cs, ns = c * 32768, n * 32768  # (exact: powers of two)
    lc.assert_close(m.scores(cs.cuda(), ns.cuda()), lc.expected(cs, ns), "gpu 16000 x32768")


def test_golden_16k(rows16):
    c, n, sr, ref = lc.golden("lsd_16k")
    assert sr == 16000
    lc.assert_close(rows16[3](c.cuda(), n.cuda()), ref, "gpu call vs reference 16k", atol=0.0)


def test_golden_8k_resampled():
    c, n, sr, ref = lc.golden("lsd_8k")
    m = LSD(8000, use_gpu=True)
    cg, ng = c.cuda(), n.cuda()
    c16, n16 = m.prepare_inputs(cg, ng)
    assert c16.shape == (4, 48000)
    want = lc.expected(c16, n16)
    got = m(cg, ng)
    lc.assert_close(got, want, "gpu call 8k vs definition on the resampled rows")
    lc.assert_close(m.scores(cg, ng, sample_rate=8000), want, "gpu scores 8k")
    lc.assert_close(got, ref, "gpu call vs reference 8k", rtol=lc.RTOL_8K, atol=0.0)


def test_gain_cases(rows16):
    x, y = lc.gain_batch()
    lc.assert_close(rows16[3].scores(x.cuda(), y.cuda()), lc.expected(x, y), "gpu gain")


def test_edge_semantics(rows16):
    c, n = lc.edge_rows()
    m = rows16[3]
    got = m.scores(c.cuda(), n.cuda())
    lc.assert_close(got, lc.expected(c, n), "gpu edge rows")
    g = got.double().cpu().numpy()
    assert abs(g[0]) <= lc.ATOL
    assert abs(g[1] - lc.LN1E8) <= 1e-5 * lc.LN1E8 and abs(g[3] - lc.LN1E8) <= 1e-5 * lc.LN1E8
    assert np.isfinite(g[2]) and g[2] > 20
    assert abs(g[4]) <= lc.ATOL and abs(g[5]) <= lc.ATOL
    # n = 0 in a ragged list, and a batch of no samples
    lens = [0, 1, 255, 256, 700]
    c, n = lc.speech_rows(len(lens), 700, seed=13)
    res = m([c[b, :k].cuda() for b, k in enumerate(lens)], [n[b, :k].cuda() for b, k in enumerate(lens)])
    assert [tuple(r) for r in res] == [LSD.KEYS] * len(lens)
    lc.assert_close(res, lc.expected(c, n, lens), "gpu ragged list")
    lc.assert_close(m.scores(c[:, :0].cuda(), n[:, :0].cuda()), np.full(len(lens), lc.LN1E8), "gpu no samples")


def test_frame_and_chunk_edges(rows16):
    lib = _native.load_lsd()
    C = lib.fsem_lsd_chunk()
    cap = 2 * C + 257
    lens = [0, 1, 255, 256, 257, 511, 512, 513, C - 1, C, C + 1, C + 255, C + 256, 2 * C + 257]
    c, n = lc.speech_rows(len(lens), cap, seed=17)
    want = lc.expected(c, n, lens)
    # whatever the memory past a row's length holds
    cp, npad = c.clone(), n.clone()
    for b, k in enumerate(lens):
        cp[b, k:] = float("nan")
        npad[b, k:] = 1e30
    m = rows16[3]
    cg, ng = cp.cuda(), npad.cuda()
    got = m.scores(cg, ng, lengths=lens)
    lc.assert_close(got, want, "gpu frame and chunk edges")
    mask = torch.arange(cap)[None] < torch.tensor(lens)[:, None]
    cq = torch.where(mask, c, torch.tensor(1e30))
    nq = torch.where(mask, n, torch.tensor(float("nan")))
    assert_bitwise(m.scores(cq.cuda(), nq.cuda(), lengths=lens), got, "the padding swapped between the operands")
    for b, k in enumerate(lens):
        assert lib.fsem_lsd_frames(k) == 1 + k // 256
        if k == 0:
            continue  # (a batch needs a sample; the row's value is checked above)
        alone = m.scores(cg[b:b + 1, :k], ng[b:b + 1, :k])
        assert_bitwise(got[b:b + 1], alone, f"row {b} (n = {k}) alone")


def test_nonfinite_rows():
    pm.nonfinite_rows("LSD")


def test_past_grid_limit():
    pm.past_grid_limit("LSD")


def test_cpu_mode_agrees():
    pm.cpu_mode_agrees("LSD")


def test_abi_refuses_before_launch():
    pm.refuses_before_launch("LSD")
