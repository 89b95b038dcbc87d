"""SRMR without a GPU: the two C entries (declared, exported, bound; their refusals, answered on the
host before any launch), the package's CPU mode against the float64 statement of the definition
(tests/srmr_cases.py), the class API, the NaN conventions, and the distance between the definition
and SRMRpy's Hilbert-envelope form."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SRMR, _build, _cpu, _native

from . import contract
from . import srmr_cases as sc

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# The largest relative |SRMRpy form - definition| measured on the cases' rows (16 kHz, the 1 s
# reverberated row): between two float64 formulations, no engine involved.
HILBERT_LARGEST = 6.232e-3


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


def test_entries_are_declared_exported_and_bound(lib):
    contract.entries_are_declared_exported_and_bound(lib, "fsem_srmr_", ("fsem_srmr_channels", "fsem_srmr_f32"))
    assert "srmr.hip" in _build.SOURCES
    assert [lib.fsem_srmr_channels(sr) for sr in (8000, 16000, 0, 4000, 11025, 22050, 44100, 48000)] == \
        [23, 23, 0, 0, 0, 0, 0, 0]
    assert sc.NCH == SRMR.CHANNELS == 23 and sc.NMOD == SRMR.MODS == 8 and sc.TILE == SRMR.TILE


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(16), None
    B, L, big = 3, 8000, (1 << 29) + 1
    call = contract.by_name(lib.fsem_srmr_f32, "deg batch length ld lengths sr energies srmr", null)
    ok = dict(deg=p, batch=B, length=L, ld=L, lengths=null, energies=p, srmr=p)
    for sr in (8000, 16000):
        contract.refusals(call, dict(ok, sr=sr), contract.nulled(_native.FSEM_EINVAL, "deg energies srmr")
                          + contract.each(_native.FSEM_EINVAL, dict(batch=-1), dict(length=-1), dict(ld=L - 1),
                                          dict(length=big, ld=big))
                          # nothing to score, nothing launched
                          + contract.each(_native.FSEM_OK, dict(batch=0), dict(batch=0, length=0, ld=0)))
    for sr in (0, 4000, 11025, 22050, 44100, 48000):
        contract.refusals(call, dict(ok, sr=sr), [({}, _native.FSEM_ERATE),
                                                  (dict(deg=null), _native.FSEM_EINVAL)])  # (arguments first)


@pytest.mark.parametrize("sr", [8000, 16000])
def test_cpu_mode_against_the_restatement(sr):
    """1 s and 2 s rows of every kind; both sides float64 by the same recipe."""
    for x, f64, _ in sc.parity_rows(sr):
        score, A = _cpu.srmr(torch.from_numpy(x.copy())[None], sr, return_energies=True)
        print(f"cpu mode {sr} n = {len(x)}: SRMR {float(score[0]):.6f}, statement {f64[0]:.6f}")
        np.testing.assert_allclose(float(score[0]), f64[0], rtol=1e-9)
        np.testing.assert_allclose(A[0].numpy(), f64[1], rtol=1e-9, atol=1e-9 * f64[1].max())


def test_filters_of_the_definition():
    for sr in (8000, 16000):
        cf = sc.centre_freqs(sr)
        assert len(cf) == 23 and (np.diff(cf) < 0).all() and abs(cf[-1] - 125.0) < 1e-9
        p, g, erb, mb, ma, L = _cpu._srmr_filters(sr)
        np.testing.assert_allclose(erb, sc.erb(cf), rtol=1e-12)
        b, a, Ls = sc.mod_filters(sr)
        np.testing.assert_allclose(mb, b, rtol=1e-12, atol=0)
        np.testing.assert_allclose(ma, a, rtol=1e-12, atol=0)
        np.testing.assert_allclose(L, Ls, rtol=1e-12)
        assert (1 - np.abs(np.roots(a[0])) < 4e-4 * 16000 / sr).all()  # the 4 Hz filter's poles hug the unit circle
        assert _cpu.srmr_geometry(sr) == sc.geometry(sr) == ((512, 2048) if sr == 8000 else (1024, 4096))


def test_class_api_and_ragged_rows():
    import fast_se_metrics
    import fast_speech_enhancement_metrics_amd as pkg
    assert pkg.SRMR is SRMR and "SRMR" in pkg.__all__
    assert fast_se_metrics.__all__ == ["STOI", "PESQ"]  # (the reference has no such metric)
    assert SRMR.KEYS == ("SRMR",) and SRMR.higher_is_better is True
    for sr in (4000, 11025, 22050, 48000):
        with pytest.raises(NotImplementedError, match="8000 or 16000"):
            SRMR(sr)
    sr = 8000
    m = SRMR(sr)
    assert (m.hop_length, m.win_length) == (512, 2048) and m.frames_of(2047) == 0 and m.frames_of(2560) == 2
    refs = sc.edge_rows(sr)[:5]
    lens = [len(r[0]) for r in refs]
    x = torch.zeros(len(refs), max(lens))
    for b, r in enumerate(refs):
        x[b, :lens[b]] = torch.from_numpy(r[0].copy())
    full = m.scores(x)
    assert full.dtype == torch.float32 and full.shape == (5,)
    s, A = m.scores(x, return_energies=True)
    assert A.shape == (5, 23, 8) and A.dtype == torch.float64
    np.testing.assert_array_equal(s.numpy(), full.numpy())
    res = m(None, x)
    assert [tuple(r) for r in res] == [("SRMR",)] * 5
    for b, r in enumerate(res):
        np.testing.assert_array_equal(np.float32(r["SRMR"]), full[b].numpy())
    assert m(x, x) == res  # (a clean argument is shape-checked only)
    with pytest.raises(Exception, match="same shape"):
        m(x[:, :-1], x)
    # ragged: lengths= and lists of utterances score each row as the unpadded row alone
    poisoned = x.clone()
    for b, k in enumerate(lens):
        poisoned[b, k:] = float("nan")
    ragged, RA = m.scores(poisoned, lengths=lens, return_energies=True)
    lists = m(None, [x[b, :k] for b, k in enumerate(lens)])
    for b, k in enumerate(lens):
        alone, AA = m.scores(x[b:b + 1, :k], return_energies=True)
        np.testing.assert_array_equal(ragged[b].numpy(), alone[0].numpy())
        np.testing.assert_array_equal(RA[b].numpy(), AA[0].numpy())
        np.testing.assert_array_equal(np.float32(lists[b]["SRMR"]), alone[0].numpy())
        if sc.frames_of(k, sr):
            np.testing.assert_allclose(float(alone[0]), refs[b][1][0], rtol=1e-6)
    assert math.isnan(lists[0]["SRMR"]) and lens[0] == 2047  # no frame
    empty = m.scores(torch.zeros(2, 0), return_energies=True)
    assert torch.isnan(empty[0]).all() and empty[0].shape == (2,) and empty[1].shape == (2, 23, 8)
    assert m.scores(torch.zeros(0, 4000)).shape == (0,)


def test_nan_conventions():
    sr = 16000
    wi, wl = sc.geometry(sr)
    x = torch.from_numpy(np.stack([sc.white(sr, wl + wi, seed) for seed in (1, 2, 3, 4)]))
    base = _cpu.srmr(x, sr)
    assert torch.isfinite(base).all()
    assert torch.isnan(_cpu.srmr(x[:, :wl - 1], sr)).all()  # F = 0
    assert torch.isfinite(_cpu.srmr(x[:, :wl], sr)).all()  # F = 1
    y = x.clone()
    y[1] = 0.0  # digitally silent: 0 / 0
    y[2, wl + wi - 1] = float("inf")  # the row's last sample
    y[3, 17] = float("nan")
    got, A = _cpu.srmr(y, sr, return_energies=True)
    assert torch.isnan(got[1:]).all() and (A[1] == 0).all()
    np.testing.assert_array_equal(got[0].numpy(), base[0].numpy())  # the neighbour is untouched
    for form in ("f64", "c64"):
        assert math.isnan(sc.srmr(y[1].numpy(), sr, form)[0]) and math.isnan(sc.srmr(y[3].numpy(), sr, form)[0])


@pytest.mark.parametrize("sr", [8000, 16000])
def test_hilbert_form_against_the_definition(sr):
    """SRMRpy's envelopes (|hilbert| of Slaney's real cascade) against the analytic gammatone's, both
    float64, on the cases' rows: what the one stated change of the definition costs."""
    worst = 0.0
    for name, refs in (("parity", sc.parity_rows(sr)), ("edge", sc.edge_rows(sr))):
        for x, f64, _ in refs:
            if not np.isfinite(f64[0]):
                continue
            d = sc.rel(sc.srmr(x, sr, "hilbert")[0], f64[0])
            print(f"hilbert form {sr} {name} n = {len(x)}: relative difference {d:.3e}")
            worst = max(worst, d)
    print(f"hilbert form {sr}: largest {worst:.3e} (bar {2 * HILBERT_LARGEST:.3e})")
    assert worst <= 2 * HILBERT_LARGEST
