"""SpectralMeasures without a GPU: the C entry's refusals (answered on the host, before any launch),
the package's CPU mode against the float64 statement of the definitions (tests/spectral_cases.py),
closed forms, the class API and the generated tables."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SpectralMeasures, _build, _cpu, _native

from . import sdr_cases
from . import spectral_cases as sp
from . import contract

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(REPO, "fast_speech_enhancement_metrics_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


def test_order_and_frames(lib):
    assert [lib.fsem_spectral_order(sr) for sr in (8000, 16000, 0, 4000, 11025, 22050, 48000)] == [10, 16, 0, 0, 0, 0, 0]
    for sr in (8000, 16000):
        assert lib.fsem_spectral_order(sr) == sp.order(sr) == _cpu.composite_order(sr)
        for n in (0, 479, 480, 599, 600, 16000):
            assert lib.fsem_sdr_frames(n, sr) == sp.frames_of(n, sr)


def test_abi_refuses_before_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH; dummy non-null pointers are never read)
    p, null = ctypes.c_void_p(16), None
    B, L, big = 3, 8000, (1 << 29) + 1
    EINVAL, OK = _native.FSEM_EINVAL, _native.FSEM_OK
    call = contract.by_name(lib.fsem_spectral_f32, "ref deg batch length ld lengths sr frames ldf fw cd is_", null)
    ok = dict(ref=p, deg=p, batch=B, length=L, ld=L, lengths=null, frames=p, fw=p, cd=p, is_=p)
    for sr in (8000, 16000):
        F = lib.fsem_sdr_frames(L, sr)
        contract.refusals(call, dict(ok, sr=sr, ldf=F), contract.nulled(EINVAL, "ref deg frames fw cd is_")
                          + contract.each(EINVAL, dict(ldf=F - 1), dict(ldf=0),
                                          dict(length=0, ld=0, ldf=0),  # ldf >= max(F, 1)
                                          dict(batch=-1), dict(length=-1), dict(ld=L - 1),
                                          dict(length=big, ld=big, ldf=1 << 29))
                          # nothing to score, nothing launched
                          + contract.each(OK, dict(batch=0), dict(batch=0, length=0, ld=0, ldf=1)))
    for sr in (0, 4000, 11025, 22050, 44100, 48000):
        contract.refusals(call, dict(ok, sr=sr, ldf=L), [({}, _native.FSEM_ERATE)])


def test_entries_are_declared_and_bound():
    header = open(os.path.join(REPO, "include", "fsem.h")).read()
    for name in ("fsem_spectral_order", "fsem_spectral_f32"):
        assert name in _native.SIGNATURES and f"{name}(" in header
    assert ctypes.c_size_t not in _native.SIGNATURES["fsem_spectral_f32"][1]  # no workspace
    assert "spectral.hip" in _build.SOURCES


@pytest.mark.parametrize("sr", [8000, 16000])
def test_cpu_mode_against_the_restatement(sr):
    c, n = sp.parity_rows(sr)
    want = sp.expected(c, n, sr)
    got = sp.to_np(_cpu.spectral(c, n, sr))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8)  # (both float64: summation orders differ)
    ce, ne, lens = sp.edge_rows(sr)
    m = SpectralMeasures(sr)
    out = m.scores(ce, ne, lengths=lens, return_frames=True)
    sp.assert_scores(out, ce, ne, sr, lengths=lens, what=f"cpu edges {sr}", atol=sp.ATOL_EDGE)
    fr = out[3].numpy()
    assert fr.shape == (3, len(lens), sp.frames_of(max(lens), sr))
    for b, k in enumerate(lens):
        F = sp.frames_of(k, sr)
        assert np.isnan(fr[:, b, F:]).all()
        fw, cd, is_ = sp.frame_values(ce[b, :k].numpy(), ne[b, :k].numpy(), sr)
        np.testing.assert_allclose(fr[:, b, :F], np.stack([fw, cd, is_]), rtol=1e-6, atol=1e-5)


@pytest.mark.parametrize("sr", [8000, 16000])
def test_closed_forms(sr):
    """Identical rows: e_s = e_s^, err at its floor 2^-52 and every band far above it: 35; equal
    cepstra: 0; IS = 1 + ln 1 - 1 = 0.  s^ = alpha s (alpha a power of two: exact in float32):
    R_s^ = alpha^2 R_s, so Levinson gives the same A and the same cepstrum (CD = 0), E_s^ = alpha^2 E_s
    and A_s^ T_s A_s^' = E_s: IS_f = 1 / alpha^2 + ln alpha^2 - 1 in every frame (clamped to 100); the
    normalised magnitudes are equal: fwSegSNR = 35."""
    c, _ = sp.parity_rows(sr)
    for impl in (lambda a, b: sp.expected(a, b, sr), lambda a, b: sp.to_np(_cpu.spectral(a, b, sr))):
        got = impl(c, c)
        np.testing.assert_array_equal(got[0], 35.0)
        np.testing.assert_array_equal(got[1], 0.0)
        np.testing.assert_allclose(got[2], 0.0, rtol=0, atol=1e-9)
        for alpha in (0.5, 2.0, 0.0625):
            got = impl(c, c * alpha)
            want_is = min(100.0, 1 / alpha ** 2 + math.log(alpha ** 2) - 1)
            np.testing.assert_array_equal(got[0], 35.0)
            np.testing.assert_allclose(got[1], 0.0, rtol=0, atol=1e-9)
            np.testing.assert_allclose(got[2], want_is, rtol=0, atol=1e-8)


def test_nan_conventions():
    sr = 16000
    hop, win = sdr_cases.hop_win(sr)
    c, n = sp.silent_head_rows(sr, win + 2 * hop)  # frames 0 .. 2 are silent in the clean row
    for fw, cd, is_ in (sp.frame_values(c[0].numpy(), n[0].numpy(), sr),
                        _cpu.spectral(c, n, sr, return_frames=True)[3][:, 0].numpy()):
        assert np.isnan(fw[:3]).all() and np.isnan(cd[:3]).all() and np.isnan(is_[:3]).all()
        assert np.isfinite(fw[3:]).all() and np.isfinite(cd[3:]).all() and np.isfinite(is_[3:]).all()
    F = sp.frames_of(c.shape[1], sr)
    assert F - sp.trimmed_count(F) >= 3  # the three NaN frames are trimmed away
    got = sp.to_np(_cpu.spectral(c, n, sr))
    assert np.isnan(got[0, 0]) and np.isfinite(got[1:, 0]).all()
    np.testing.assert_allclose(got, sp.expected(c, n, sr), rtol=0, atol=1e-8)
    # a silent denoised frame: err = e_s^2 in every band, so every log ratio is 0
    fw = sp.frame_values(n[0, :win].numpy(), np.zeros(win), sr)[0]
    assert fw[0] == 0.0
    assert float(_cpu.spectral(n[:, :win], torch.zeros(1, win), sr)[0]) == 0.0
    # non-finite samples, also in the tail that no frame covers; rows too short for a frame
    c2, n2 = sp.parity_rows(sr)
    n2 = n2.clone()
    n2[1, 5000] = float("nan")
    n2[2, -1] = float("inf")
    assert sp.frames_of(n2.shape[1], sr) == sp.frames_of(n2.shape[1] - 1, sr)  # (the last sample is in no frame)
    got = sp.to_np(_cpu.spectral(c2, n2, sr))
    assert np.isnan(got[:, 1:3]).all() and np.isfinite(got[:, [0, 3]]).all()
    assert all(torch.isnan(v).all() for v in _cpu.spectral(c2[:, :win - 1], n2[:, :win - 1], sr))


def test_class_api():
    import fast_se_metrics
    import fast_speech_enhancement_metrics_amd as pkg
    assert pkg.SpectralMeasures is SpectralMeasures and "SpectralMeasures" in pkg.__all__
    assert fast_se_metrics.__all__ == ["STOI", "PESQ"]  # (the reference has no such metric)
    assert SpectralMeasures.KEYS == ("fwSegSNR", "CD", "IS")
    assert SpectralMeasures.higher_is_better == {"fwSegSNR": True, "CD": False, "IS": False}
    for sr in (4000, 11025, 22050, 48000):
        with pytest.raises(NotImplementedError, match="8000 or 16000"):
            SpectralMeasures(sr)
    sr = 8000
    m = SpectralMeasures(sr)
    assert (m.hop_length, m.win_length, m.lpc_order) == (60, 240, 10)
    c, n = sp.parity_rows(sr)
    lens = [c.shape[1], 3000, 239, 1000]
    cols = m.scores(c, n)
    assert len(cols) == 3 and all(v.dtype == torch.float32 and v.shape == (4,) for v in cols)
    out = m.scores(c, n, return_frames=True)
    assert len(out) == 4 and out[3].shape == (3, 4, sp.frames_of(c.shape[1], sr)) and out[3].dtype == torch.float32
    for a, b in zip(out[:3], cols):
        np.testing.assert_array_equal(a.numpy(), b.numpy())
    res = m(c, n)
    assert [tuple(r) for r in res] == [SpectralMeasures.KEYS] * 4
    for b, r in enumerate(res):
        for k, key in enumerate(SpectralMeasures.KEYS):
            np.testing.assert_array_equal(np.float32(r[key]), cols[k][b].numpy())
    # ragged: lengths= and lists of utterances score each row as the row alone
    ragged = m.scores(c, n, lengths=lens)
    lists = m([c[b, :k] for b, k in enumerate(lens)], [n[b, :k] for b, k in enumerate(lens)])
    for b, k in enumerate(lens):
        alone = m.scores(c[b:b + 1, :k], n[b:b + 1, :k])
        for j, key in enumerate(SpectralMeasures.KEYS):
            np.testing.assert_array_equal(ragged[j][b].numpy(), alone[j][0].numpy())
            np.testing.assert_array_equal(np.float32(lists[b][key]), alone[j][0].numpy())
    assert all(math.isnan(v) for v in lists[2].values())  # 239 samples: no frame
    empty = m.scores(torch.zeros(2, 0), torch.zeros(2, 0), return_frames=True)
    assert all(torch.isnan(v).all() and v.shape == (2,) for v in empty[:3]) and empty[3].shape == (3, 2, 0)
    with pytest.raises(Exception, match="same shape"):
        m.scores(c, n[:, :-1])


def test_committed_tables_equal_the_generator(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("fsem_gen_tables", os.path.join(CSRC, "gen_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    monkeypatch.setattr(gen, "HERE", str(tmp_path))
    gen.main()
    made = open(os.path.join(str(tmp_path), "fsem_tables.inc")).read()
    assert made == open(os.path.join(CSRC, "fsem_tables.inc")).read()
    for name in ("kSpecWin8k[240]", "kSpecWin16k[480]", "kSpecG8k[25][32]", "kSpecG16k[25][32]", "kSpecJ08k[25]",
                 "kSpecJ016k[25]", "kSpecTw[512][2]"):
        assert name in made, name
    # the sparse tables hold the restatement's filters, rounded once to float32
    for sr in (8000, 16000):
        w, g, j0 = gen.spectral_tables(sr)
        full = sp.filters(sr)
        H = full.shape[1]
        for i in range(25):
            dense = np.zeros(H)
            for q in range(gen.SPEC_GW):
                if 0 <= j0[i] + q < H:
                    dense[j0[i] + q] = g[i, q]
            np.testing.assert_array_equal(dense, full[i])
