"""The stage surface on the GPU (engine stage entries) against the reference's golden intermediates:
Bark bands (fsem_pesq_front_f32), symmetric / asymmetric distances and per-frame disturbances
(fsem_pesq_distances_f32, the PESQ back end's intermediates -- VERDICT r2 weak #3), and the
drop-in stage methods that route through them.

Bars: distances 5e-3 absolute (MOS = 4.5 - 0.1 sym - 0.0309 asym: <= 6.5e-4 in MOS; the
reference's own float32 order-10 IIR moves its Bark bands by up to ~1e-3 relative, DESIGN.md
section 2); per-frame symmetric disturbances 2e-2 absolute on the 0..45 scale, asymmetric ones
3e-2 for 99 % of frames -- a frame whose asymmetry factor ((n + 50) / (c + 50))^1.2 sits at its
threshold 3 (PESQ.py:214-216) jumps by w_k d_k 3 between any two float32 evaluations; Bark bands
5e-3 of the row's peak.
"""
import numpy as np
import pytest
import torch

from tests.conftest import PESQ_CASES, load_golden
from tests import contract

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return contract.device()


@pytest.mark.parametrize("name", PESQ_CASES)
def test_back_end_distances_match_reference(dev, name):
    from fast_se_metrics import PESQ
    g = load_golden(name)
    m = PESQ(16000, use_gpu=True)
    sym, asym, frames = m.frame_disturbances(torch.from_numpy(g["clean_f"]).to(dev), torch.from_numpy(g["noisy_f"]).to(dev))
    sym, asym, frames = sym.double().cpu().numpy(), asym.double().cpu().numpy(), frames.double().cpu().numpy()
    print(name, "sym", np.abs(sym - g["sym"]).max(), "asym", np.abs(asym - g["asym"]).max())
    np.testing.assert_allclose(sym, g["sym"], rtol=0, atol=5e-3)
    np.testing.assert_allclose(asym, g["asym"], rtol=0, atol=5e-3)
    F = g["sym_frames"].shape[1]
    assert frames.shape[2] == F
    ds = np.abs(frames[:, 0] - g["sym_frames"])
    da = np.abs(frames[:, 1] - g["asym_frames"])
    print(name, "frames: max", ds.max(), da.max(), "p99", np.quantile(ds, 0.99), np.quantile(da, 0.99))
    assert ds.max() < 2e-2 and np.quantile(da, 0.99) < 3e-2
    # the MOS mapping of the distances is the engine's score
    mos = 0.999 + 4 / (1 + np.exp(-1.3669 * (4.5 - 0.1 * sym - 0.0309 * asym) + 3.8224))
    got = PESQ(16000, use_gpu=True).scores(torch.from_numpy(g["clean_f"]).to(dev), torch.from_numpy(g["noisy_f"]).to(dev))
    np.testing.assert_allclose(mos, got.double().cpu().numpy(), atol=2e-6, rtol=0)


def test_distances_ragged_rows(dev):
    """Per-row lengths: each row's distances are its unpadded row's; rows under 20 frames NaN."""
    from fast_se_metrics import PESQ
    g = load_golden("varlen_16k")
    m = PESQ(16000, use_gpu=True)
    c, n = torch.from_numpy(g["clean_f"]).to(dev), torch.from_numpy(g["noisy_f"]).to(dev)
    lens = torch.from_numpy(g["lengths"]).to(dev)
    sym, asym, _ = m.frame_disturbances(c, n, lengths=lens)
    mos = 0.999 + 4 / (1 + torch.exp(-1.3669 * (4.5 - 0.1 * sym.double() - 0.0309 * asym.double()) + 3.8224))
    mos = mos.cpu().numpy()
    assert np.array_equal(np.isnan(mos), np.isnan(g["pesq"]))
    ok = ~np.isnan(g["pesq"])
    np.testing.assert_allclose(mos[ok], g["pesq"][ok], atol=5e-3, rtol=0)


@pytest.mark.parametrize("name", ["pesq_3s", "pesq_ragged"])
def test_stage_methods_on_gpu(dev, name):
    from fast_se_metrics import PESQ
    g = load_golden(name)
    m = PESQ(16000, use_gpu=True)
    c, n = torch.from_numpy(g["clean_f"]).to(dev), torch.from_numpy(g["noisy_f"]).to(dev)
    ce, ne = m.equalize_ranges(c, n)
    bark = m.get_bark_bands(torch.cat([ce, ne], 0)).cpu().numpy()
    ref = g["bark"].astype(np.float64)
    assert bark.shape == ref.shape
    rel = (np.abs(bark - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))).max()
    assert rel < 5e-3, rel
    aligned = m.align_level(torch.cat([ce, ne], 0)).double()
    x = torch.cat([ce, ne], 0).double()
    scale = ((aligned * x).sum(1) / x.square().sum(1)).cpu().numpy()
    np.testing.assert_allclose(scale, g["level_scale"], rtol=3e-3)
    sym, asym = m.get_disturbances(c, n)
    np.testing.assert_allclose(sym.double().cpu().numpy(), g["sym"], rtol=0, atol=5e-3)
    np.testing.assert_allclose(asym.double().cpu().numpy(), g["asym"], rtol=0, atol=5e-3)
    B = c.shape[0]
    bt = torch.from_numpy(bark).to(dev)
    ec, en = m.equalize_bark_bands(bt[:B], bt[B:])
    assert ec.is_cuda and ec.shape == en.shape


def test_stoi_stage_methods_on_gpu(dev):
    from fast_se_metrics import STOI
    g = load_golden("stoi_10k")
    m = STOI(10000, use_gpu=True)
    c, n = torch.from_numpy(g["clean_f"]).to(dev), torch.from_numpy(g["noisy_f"]).to(dev)
    cs, ns, lens = m.remove_silent_frames(c, n)
    assert ((lens // 128 - 1).cpu().numpy() == g["kept"]).all()
    segs = m.compute_segments(torch.cat([cs, ns], 0), torch.cat([lens, lens], 0))
    assert segs[0].is_cuda
    s, e = m.compute_stoi(c, n)
    np.testing.assert_allclose(s.cpu().numpy(), g["stoi"], atol=5e-4, rtol=0)
    np.testing.assert_allclose(e.cpu().numpy(), g["estoi"], atol=5e-4, rtol=0)


def test_stage_dtypes_and_devices_match_reference(dev):
    """The reference's stage outputs (PESQ.py:92-140): align_level and pre_emphasize float32 (its
    lfilter keeps the input dtype), get_bark_bands float64 (BarkFilterBank.forward multiplies by
    the float64 pow_dens_correction, bark.py:132,204); every one on the input's device -- on a
    use_gpu=True metric pre_emphasize never leaves the device.  Rows shorter than one 512-sample
    frame still level-align (the reference filters any length)."""
    from fast_se_metrics import PESQ
    from oracle import ta
    m = PESQ(16000, use_gpu=True)
    g = load_golden("pesq_3s")
    x = torch.from_numpy(g["clean_f"]).to(dev)
    al = m.align_level(x.clone())
    assert al.dtype == torch.float32 and al.is_cuda
    pe_in = al.clone()
    pe = m.pre_emphasize(pe_in)
    assert pe.dtype == torch.float32 and pe.is_cuda
    # bitwise the torchaudio-order float32 lfilter (oracle/c/lfilter_f32.c) of the tapered rows
    # (pre_emphasize tapers its argument in place, as the reference)
    want = ta.lfilter(pe_in.cpu().numpy(), np.array([1.0, -1.9444777, 0.94597794], np.float32),
                      np.array([2.740826, -5.4816519, 2.740826], np.float32))
    np.testing.assert_array_equal(pe.cpu().numpy(), want)
    bark = m.get_bark_bands(x.clone())
    assert bark.dtype == torch.float64 and bark.is_cuda
    short = torch.randn(3, 300, device=dev)
    s_al = m.align_level(short)
    assert s_al.dtype == torch.float32 and s_al.is_cuda and torch.isfinite(s_al).all()
    cpu = PESQ(16000).align_level(short.cpu())
    np.testing.assert_allclose(s_al.cpu().numpy(), cpu.numpy(), rtol=1e-6, atol=0)
