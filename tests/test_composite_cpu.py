"""Composite metric (CSIG, CBAK, COVL with PESQ, LLR, WSS, SegSNR) without a GPU: the CPU mode
against the float64 statement of the definitions (tests/composite_cases.py), the lowest-95 % rule,
the peak search's quirk, silent and non-finite rows, the drop-in call, the C-ABI's host-side
validation (no launch), copying and pickling."""
import ctypes
import math

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import Composite

from . import composite_cases as cc
from . import sdr_cases as sc
from . import contract
from . import pair_metrics as pm


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.fixture(scope="module")
def clib(lib):
    """libfsem_composite.so (include/fsem_composite.h), built with libfsem.so."""
    from fast_speech_enhancement_metrics_amd import _native
    return _native.load_composite()


@pytest.mark.parametrize("sr", [8000, 16000])
def test_cpu_mode_matches_definition(sr):
    c, n = cc.parity_rows(sr)
    got = Composite(sr, use_gpu=False).scores(c, n)
    assert all(g.dtype == torch.float32 and g.shape == (4,) for g in got)
    cc.assert_scores(got, c, n, sr, what=f"cpu {sr}")
    assert np.isfinite(cc.to_np(got)).all()


@pytest.mark.parametrize("sr", [8000, 16000])
def test_identical_and_scaled_rows(sr):
    c, _ = cc.parity_rows(sr)
    m = Composite(sr)
    csig, cbak, covl, pesq, llr, wss, seg = (v.numpy() for v in m.scores(c, c))
    assert (llr == 0).all() and (wss == 0).all() and (csig == 5).all()
    # LLR and WSS are scale-invariant while the band energies stay above the floor
    want = cc.expected_llr_wss(c, 0.25 * c, sr)
    assert np.abs(want).max() <= 1e-9
    got = cc.to_np(m.scores(c, 0.25 * c))
    assert np.abs(got[4]).max() <= 1e-9 and np.abs(got[5]).max() <= 1e-9


@pytest.mark.parametrize("F", [1, 10, 30])
def test_lowest_95_percent_rule(F):
    sr = 16000
    c, n = cc.frames_row(F, sr)
    llr, wss = cc.frame_values(c[0].numpy(), n[0].numpy(), sr)
    assert len(llr) == F
    K = cc.trimmed_count(F)
    assert K == {1: 1, 10: 10, 30: 29}[F]  # round(0.95 F), halves up: 28.5 -> 29
    want = np.array([[np.sort(llr)[:K].mean()], [np.sort(wss)[:K].mean()]])
    if F == 30:
        assert abs(np.sort(llr)[:28].mean() - want[0, 0]) > 1e-4  # (28 frames would be told apart)
    lens = [c.shape[1]]
    got = cc.to_np(Composite(sr).scores(c, n, lengths=lens))
    cc.assert_scores(got, c, n, sr, lengths=lens, what=f"cpu F={F}", want=want)
    assert math.isnan(got[3, 0]) == (F < 20 * 256 // 120)  # (PESQ needs 20 of its own frames)


def test_no_frame_is_nan():
    sr = 16000
    hop, win = sc.hop_win(sr)
    c, n, = cc.frames_row(2, sr)
    lens = [win - 1]
    got = cc.to_np(Composite(sr).scores(c, n, lengths=lens))
    assert np.isnan(got[4:]).all() and np.isnan(got).all()
    assert np.isnan(cc.expected_llr_wss(c, n, sr, lengths=lens)).all()
    # the whole-batch form of a row too short for PESQ: the PESQ class's exception
    with pytest.raises(RuntimeError, match="size is 20"):
        Composite(sr).scores(c, n)


def test_peak_search_quirk():
    # rising to band 3, falling to band 7, flat to 9, rising to 12, falling to the end
    e = np.array([10, 20, 30, 40, 35, 30, 25, 20, 20, 20, 30, 40, 50, 45, 40, 35, 30, 25, 20, 15, 10, 5, 4, 3, 2.0])
    pk = cc.peaks(e)
    # a rising band looks right for the first slope m that does not rise and takes e[m - 1]: the
    # quirk -- that is the band below the peak (30 under the peak of 40, 40 under the peak of 50)
    assert list(pk[:3]) == [30, 30, 30] and list(pk[9:12]) == [40, 40, 40]
    # a falling (or flat) band looks left for the last rising slope m and takes e[m + 1]: the peak
    assert list(pk[3:9]) == [40] * 6 and list(pk[12:]) == [50] * 12
    # a vector that falls from band 0 runs off the left end and takes e[0]; one that rises to the
    # last band takes e[23], not the last band
    assert list(cc.peaks(np.arange(25, 0, -1.0))) == [25.0] * 24
    assert list(cc.peaks(np.arange(25.0))) == [23.0] * 24
    from fast_speech_enhancement_metrics_amd import _cpu
    for v in (e, np.arange(25.0), np.arange(25, 0, -1.0)):
        np.testing.assert_array_equal(_cpu._nearest_peaks(torch.from_numpy(v)[None]).numpy()[0], cc.peaks(v))


@pytest.mark.parametrize("zeroed,nan_frames,finite", [(1200, 7, True), (3000, 22, False)])
def test_silent_clean_head(zeroed, nan_frames, finite):
    sr = 16000
    c, n = cc.silent_head_rows(sr, zeroed)
    llr, wss = cc.frame_values(c[0].numpy(), n[0].numpy(), sr)
    F = len(llr)
    assert F == 197 and F - cc.trimmed_count(F) == 10
    assert int(np.isnan(llr).sum()) == nan_frames and np.isfinite(wss).all()
    want = cc.expected_llr_wss(c, n, sr)
    assert np.isfinite(want[0, 0]) == finite and np.isfinite(want[1, 0])
    cc.assert_scores(Composite(sr).scores(c, n), c, n, sr, what=f"cpu silent head {zeroed}", want=want)


def test_nonfinite_row_is_nan_alone():
    pm.nonfinite_row_is_nan_alone("Composite")


def test_drop_in_call_key_order_and_shape_check():
    c, n = cc.parity_rows(8000)
    m = Composite(8000)
    assert m.higher_is_better and m.device == "cpu" and m.resampler(c) is c
    assert Composite.KEYS == cc.KEYS == ("CSIG", "CBAK", "COVL", "PESQ", "LLR", "WSS", "SegSNR")
    res = m(c, n)
    assert isinstance(res, list) and len(res) == 4 and [tuple(r) for r in res] == [cc.KEYS] * 4
    s = m.scores(c, n)
    for k, key in enumerate(m.KEYS):
        assert [r[key] for r in res] == [float(v) for v in s[k]]
    # lists of utterances: a row too short for PESQ is NaN there, its LLR / WSS / SegSNR are scored
    lens = [12000, 2400, 12000, 700]
    res = m([c[b, :k] for b, k in enumerate(lens)], [n[b, :k] for b, k in enumerate(lens)])
    got = np.array([[r[k] for r in res] for k in cc.KEYS])
    cc.assert_scores(got, c, n, 8000, lengths=lens, what="cpu list")
    assert np.isnan(got[3]).tolist() == [False, True, False, True] and np.isfinite(got[4:]).all()
    with pytest.raises(Exception, match="should have the same shape"):
        m(c, n[:, :-1])
    for sr in (3999, 22050, 48000, 200000):
        with pytest.raises(NotImplementedError):
            Composite(sr)
    import fast_se_metrics
    assert fast_se_metrics.__all__ == ["STOI", "PESQ"]


def test_abi_queries(lib, clib):
    for sr in (8000, 16000):
        assert clib.fsem_composite_workspace_bytes(4, 10 * sr, sr) > lib.fsem_pesq_workspace_bytes(4, 160000) > 0
        assert clib.fsem_composite_chunk(sr) == 16 * lib.fsem_sdr_hop(sr)
    for sr in (3999, 22050, 200000):
        assert clib.fsem_composite_workspace_bytes(4, 160000, sr) == 0 and clib.fsem_composite_chunk(sr) == 0
    assert lib.fsem_version() == 11  # (libfsem.so is as it was: the composite entries are a library of their own)


def test_abi_validation_without_launch(clib):
    from fast_speech_enhancement_metrics_amd import _native
    null, p = None, ctypes.c_void_p(16)
    outs = [f"o{k}" for k in range(7)]
    names = "ref deg batch length ld lengths sr " + " ".join(outs) + " ws ws_bytes"
    call = contract.by_name(clib.fsem_composite_f32, names, null)
    ok = dict(ref=p, deg=p, batch=4, length=160000, ld=160000, lengths=null, sr=16000, ws=p, ws_bytes=1 << 40,
              **{o: p for o in outs})
    big = (1 << 29) + 4
    half = (1 << 28) + 4  # 8 kHz rows whose 16 kHz copies would pass 2^29 samples
    contract.refusals(call, ok, contract.nulled(_native.FSEM_EINVAL, " ".join(outs)) + contract.each(  # (each output)
        _native.FSEM_EINVAL, dict(ref=null, deg=null, ws=null, ws_bytes=0, **{o: null for o in outs}), dict(batch=0),
        dict(length=0, ld=0), dict(ld=159999), dict(batch=1, length=big, ld=big, ws_bytes=1 << 62),
        dict(batch=1, length=half, ld=half, sr=8000, ws_bytes=1 << 62))
        + contract.each(_native.FSEM_ERATE, dict(sr=3999), dict(sr=22050), dict(sr=200000))
        # the whole-batch form of rows too short for PESQ: refused as fsem_pesq_wb_f32 refuses them
        + [(dict(length=4000, ld=4000), _native.FSEM_ESHORT)])
    for sr in (8000, 16000):
        size = clib.fsem_composite_workspace_bytes(4, 160000, sr)
        contract.refusals(call, dict(ok, sr=sr), contract.each(_native.FSEM_EWORKSPACE, dict(ws_bytes=16),
                                                               dict(ws_bytes=size - 1), dict(ws=null)))
