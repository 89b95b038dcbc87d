"""LSD metric without a GPU: the CPU mode against the float64 statement of the definition
(tests/lsd_cases.py) and the reference's own scores (tests/golden/lsd_*.npz), the edge semantics,
the drop-in call, the C-ABI's host-side queries and validation (no launch), copying and pickling."""
import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import LSD, _cpu

from . import lsd_cases as lc
from . import contract
from . import pair_metrics as pm


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.fixture(scope="module")
def llib(lib):
    """libfsem_lsd.so (include/fsem_lsd.h), built with libfsem.so."""
    from fast_speech_enhancement_metrics_amd import _native
    return _native.load_lsd()


@pytest.mark.parametrize("length", lc.LENGTHS)
@pytest.mark.parametrize("scale", [1.0, 32768.0])
def test_cpu_mode_matches_definition(length, scale):
    c, n = lc.speech_rows(4, length)
    c, n = c * scale, n * scale
    want = lc.expected(c, n)
    lc.assert_close(_cpu.lsd(c, n), want, f"_cpu.lsd {length} x{scale:g}")
    m = LSD(16000, use_gpu=False)
    got = m.scores(c, n)
    assert got.dtype == torch.float32 and got.shape == (4,)
    lc.assert_close(got, want, f"cpu scores {length} x{scale:g}")
    lc.assert_close(m(c, n), want, f"cpu call {length} x{scale:g}")


def test_golden_16k():
    c, n, sr, ref = lc.golden("lsd_16k")
    assert sr == 16000 and c.shape == (4, 48000)
    lc.assert_close(lc.expected(c, n), ref, "definition vs reference 16k", atol=0.0)
    lc.assert_close(_cpu.lsd(c, n), ref, "_cpu.lsd vs reference 16k", atol=0.0)
    lc.assert_close(LSD(16000, use_gpu=False)(c, n), ref, "cpu call vs reference 16k", atol=0.0)
    # int16 codes and float64 rows score as the float32 rows
    m = LSD(16000)
    assert m(c.double(), n.double()) == m(c, n)
    codes = (c * 32768).to(torch.int16), (n * 32768).to(torch.int16)
    lc.assert_close(m(*codes), lc.expected(c * 32768, n * 32768), "cpu int16")


def test_golden_8k_drop_in():
    c, n, sr, ref = lc.golden("lsd_8k")
    assert sr == 8000 and c.shape == (4, 24000)
    m = LSD(8000, use_gpu=False)
    got = m(c, n)
    # the resamplers differ: four times the deviation measured for the CPU mode (lsd_cases.py)
    lc.assert_close(got, ref, "cpu call vs reference 8k", rtol=lc.RTOL_8K, atol=0.0)
    # the score is the definition's on the rows this package resamples
    c16, n16 = m.prepare_inputs(c, n)
    assert c16.shape == (4, 48000)
    lc.assert_close(got, lc.expected(c16, n16), "cpu call 8k vs definition on the resampled rows")
    lc.assert_close(m.scores(c, n, sample_rate=8000), lc.expected(c16, n16), "cpu scores 8k")
    with pytest.raises(ValueError, match="pass sample_rate"):
        m.scores(c, n)


def test_edge_semantics():
    c, n = lc.edge_rows()
    want = lc.expected(c, n)
    got = LSD(16000, use_gpu=False).scores(c, n)
    lc.assert_close(got, want, "cpu edges")
    g = got.double().numpy()
    assert abs(g[0]) <= lc.ATOL                                          # identical rows
    assert abs(g[1] - lc.LN1E8) <= 1e-5 * lc.LN1E8 and abs(g[3] - lc.LN1E8) <= 1e-5 * lc.LN1E8  # silent clean
    assert np.isfinite(g[2]) and g[2] > 20                               # silent estimate: large, finite
    assert abs(g[4]) <= lc.ATOL and abs(g[5]) <= lc.ATOL                 # a gain is scaled away, its sign too


def test_gain_cases():
    x, y = lc.gain_batch()
    want = lc.expected(x, y)
    assert want[0] > want[1] > want[2] > 0  # (the less noise, the smaller the distance)
    lc.assert_close(LSD(16000, use_gpu=False).scores(x, y), want, "cpu gain")


def test_empty_row_in_a_ragged_list():
    lens = [0, 1, 255, 256, 700]
    c, n = lc.speech_rows(len(lens), 700, seed=13)
    want = lc.expected(c, n, lens)
    assert abs(want[0] - lc.LN1E8) < 1e-12
    m = LSD(16000, use_gpu=False)
    lc.assert_close(m.scores(c, n, lengths=lens), want, "cpu ragged")
    res = m([c[b, :k] for b, k in enumerate(lens)], [n[b, :k] for b, k in enumerate(lens)])
    lc.assert_close(res, want, "cpu ragged list")
    lc.assert_close(m(c[:, :0], n[:, :0]), np.full(len(lens), lc.LN1E8), "cpu no samples")


def test_nonfinite_row_is_nan_alone():
    pm.nonfinite_row_is_nan_alone("LSD")


def test_drop_in_call_key_order_and_shape_check():
    c, n = lc.speech_rows(3, 16000)
    m = LSD(16000)
    assert not m.higher_is_better and m.device == "cpu" and m.resampler(c) is c
    assert m.EXPECTED_SAMPLING_RATE == 16000 and (m.nfft, m.hop, m.p, m.eps) == (512, 256, 2, 1e-8)
    assert torch.equal(m.window, torch.hann_window(512))
    res = m(c, n)
    assert isinstance(res, list) and len(res) == 3 and all(isinstance(r, dict) for r in res)
    assert [tuple(r) for r in res] == [("LSD",)] * 3 == [LSD.KEYS] * 3
    s = m.scores(c, n)
    assert [r["LSD"] for r in res] == [float(v) for v in s]
    with pytest.raises(Exception, match="should have the same shape"):
        m(c, n[:, :-1])
    with pytest.raises(Exception, match="should have the same shape"):
        m.scores(c, n[:2])
    from fast_se_metrics.LSD import LSD as DropIn
    assert DropIn is LSD


# ------------------------------------------------------------------ the C-ABI, host side
def test_abi_geometry(llib):
    C = llib.fsem_lsd_chunk()
    assert C > 0 and C % 256 == 0
    for n in (0, 1, 255, 256, 257, 511, 512, 513, C - 1, C, C + 1, 160000, 1 << 29):
        assert llib.fsem_lsd_frames(n) == 1 + n // 256


def test_abi_validation_without_launch(llib):
    pm.one_output_validation(llib, "lsd")
