"""SDR metric (SI-SDR, SNR, segmental SNR) without a GPU: the CPU mode against the float64
statement of the definitions (tests/sdr_cases.py), the edge semantics, the drop-in call, the
C-ABI's host-side queries and validation (no launch), copying and pickling."""
import ctypes
import math

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SDR

from . import sdr_cases as sc
from . import contract
from . import pair_metrics as pm


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.mark.parametrize("sr", [8000, 16000, 22050, 48000])
def test_cpu_mode_matches_definition(sr):
    c, n = sc.speech_rows(3, 2 * sr, sr)
    sc.assert_close(SDR(sr, use_gpu=False).scores(c, n), sc.expected(c, n, sr), f"cpu {sr}")


def test_gain_cases():
    x, y = sc.gain_batch()
    want = sc.expected(x, y, 16000)
    # the figures the cases were chosen for (float64 definition)
    assert abs(want[0, 0] - 60.018) < 2e-3 and abs(want[1, 0] - 3.098) < 2e-3
    assert abs(want[0, 1] - 80.022) < 2e-3 and abs(want[1, 2] - 89.980) < 2e-3
    sc.assert_close(SDR(16000, use_gpu=False).scores(x, y), want, "cpu gain")


def test_zero_mean_removes_dc():
    c, n = sc.speech_rows(3, 32000, 16000)
    cd, nd = sc.dc_rows(c, n)
    plain, zm = SDR(16000, use_gpu=False), SDR(16000, use_gpu=False, zero_mean=True)
    got = zm.scores(cd, nd)
    sc.assert_close(got, sc.expected(cd, nd, 16000, zero_mean=True), "cpu zero_mean")
    # SI-SDR of the DC rows with the option = that of the offset-free rows (zero-mean speech: their own
    # mean is about 1e-4 of their rms)
    free = sc.expected(c - c.mean(1, keepdim=True), n - n.mean(1, keepdim=True), 16000)
    np.testing.assert_allclose(got[0].numpy(), free[0], rtol=0, atol=sc.ATOL_SDR)
    # SNR and SegSNR do not see the option
    off = plain.scores(cd, nd)
    np.testing.assert_array_equal(got[1].numpy(), off[1].numpy())
    np.testing.assert_array_equal(got[2].numpy(), off[2].numpy())
    assert abs(float(off[0][0]) - float(got[0][0])) > 1.0  # (the option matters on these rows)


def test_edge_semantics():
    c, n = sc.edge_rows()
    m = SDR(16000, use_gpu=False)
    si, snr, seg = (v.numpy() for v in m.scores(c, n))
    sc.assert_close((si, snr, seg), sc.expected(c, n, 16000), "cpu edges")
    assert si[0] == math.inf and snr[0] == math.inf and seg[0] == 35.0     # identical rows
    assert math.isnan(si[1]) and snr[1] == -math.inf and seg[1] == -10.0    # silent clean
    assert math.isnan(si[2]) and abs(snr[2]) < 1e-6                         # silent estimate
    assert math.isnan(si[3]) and math.isnan(snr[3]) and seg[3] == -10.0     # both silent


@pytest.mark.parametrize("sr", [16000, 22050])
def test_short_rows(sr):
    hop, win = sc.hop_win(sr)
    lens = [0, 1, win - 1, win, win + hop - 1, win + hop]
    c, n = sc.speech_rows(len(lens), win + hop, sr, seed=13)
    m = SDR(sr, use_gpu=False)
    want = sc.expected(c, n, sr, lengths=lens)
    assert np.isnan(want[:, 0]).all() and np.isnan(want[2, :3]).all() and np.isfinite(want[2, 3:]).all()
    sc.assert_close(m.scores(c, n, lengths=lens), want, f"cpu short {sr}")
    # the same rows as a list of utterances through the drop-in call
    res = m([c[b, :k] for b, k in enumerate(lens)], [n[b, :k] for b, k in enumerate(lens)])
    assert [list(r) for r in res] == [["SI-SDR", "SNR", "SegSNR"]] * len(lens)
    sc.assert_close(np.array([[r[k] for r in res] for k in SDR.KEYS]), want, f"cpu short list {sr}")


def test_drop_in_call_and_shape_check():
    c, n = sc.speech_rows(3, 16000, 16000)
    m = SDR(16000)
    assert m.higher_is_better and m.device == "cpu" and m.resampler(c) is c
    res = m(c, n)
    assert isinstance(res, list) and len(res) == 3 and all(isinstance(r, dict) for r in res)
    assert [tuple(r) for r in res] == [("SI-SDR", "SNR", "SegSNR")] * 3
    s = m.scores(c, n)
    assert all(v.dtype == torch.float32 and v.shape == (3,) for v in s)
    for k, key in enumerate(m.KEYS):
        assert [r[key] for r in res] == [float(v) for v in s[k]]
    with pytest.raises(Exception, match="should have the same shape"):
        m(c, n[:, :-1])
    with pytest.raises(Exception, match="should have the same shape"):
        m.scores(c, n[:2])
    with pytest.raises(NotImplementedError):
        SDR(3999)


def test_nonfinite_row_is_nan_alone():
    pm.nonfinite_row_is_nan_alone("SDR")


def test_abi_geometry(lib):
    for sr, hop in sc.RATES_HOP.items():
        assert lib.fsem_sdr_hop(sr) == hop == sr * 30 // 4000
        C = lib.fsem_sdr_chunk(sr)
        assert C > 0 and C % hop == 0
        win = 4 * hop
        for L in (0, 1, win - 1, win, win + hop - 1, win + hop, 10 * sr + 7):
            assert lib.fsem_sdr_frames(L, sr) == ((L - win) // hop + 1 if L >= win else 0)
        assert lib.fsem_sdr_workspace_bytes(4, 10 * sr, sr) > 0
    for sr in (3999, 200000):
        assert lib.fsem_sdr_hop(sr) == 0 and lib.fsem_sdr_chunk(sr) == 0
        assert lib.fsem_sdr_frames(160000, sr) == 0 and lib.fsem_sdr_workspace_bytes(4, 160000, sr) == 0
    assert lib.fsem_sdr_hop(4000) == 30 and lib.fsem_sdr_hop(192000) == 1440
    assert lib.fsem_version() == 11


def test_abi_validation_without_launch(lib):
    from fast_speech_enhancement_metrics_amd import _native
    null, p = None, ctypes.c_void_p(16)
    big = (1 << 29) + 4
    call = contract.by_name(lib.fsem_sdr_f32, "ref deg batch length ld lengths sr zm si snr seg ws ws_bytes", null)
    ok = dict(ref=p, deg=p, batch=4, length=160000, ld=160000, lengths=null, sr=16000, zm=0, si=p, snr=p, seg=p, ws=p,
              ws_bytes=1 << 40)
    contract.refusals(call, ok, contract.each(
        _native.FSEM_EINVAL, dict(ref=null, deg=null, si=null, snr=null, seg=null, ws=null, ws_bytes=0), dict(seg=null),
        dict(batch=0), dict(length=0, ld=0), dict(ld=159999), dict(batch=1, length=big, ld=big, ws_bytes=1 << 62))
        + contract.each(_native.FSEM_ERATE, dict(sr=3999), dict(sr=200000))
        + contract.each(_native.FSEM_EWORKSPACE, dict(ws_bytes=16), dict(ws=null)))
