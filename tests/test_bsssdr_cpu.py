"""BSSSDR metric (the reference's SDR) without a GPU: the drop-in import path, the CPU mode against
the float64 statement of the definition (tests/bsssdr_cases.py) and the reference's own scores
(tests/golden/bsssdr_*.npz), the edge semantics, the C-ABI's host-side queries and validation (no
launch), copying and pickling."""
import os
import warnings

import numpy as np
import pytest
import torch

from . import bsssdr_cases as bc
from . import contract
from . import pair_metrics as pm

GOLDEN_FILES = ("bsssdr_16k", "bsssdr_8k", "bsssdr_white")


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.fixture(scope="module")
def blib(lib):
    """libfsem_bsssdr.so (include/fsem_bsssdr.h), built with libfsem.so."""
    from fast_speech_enhancement_metrics_amd import _native
    return _native.load_bsssdr()


def test_drop_in_import_path():
    """``from fast_se_metrics.SDR import SDR`` is the reference's metric: key "SDR", its attributes."""
    from fast_se_metrics.SDR import SDR
    from fast_speech_enhancement_metrics_amd import BSSSDR
    from fast_speech_enhancement_metrics_amd import SDR as PackageSDR
    import fast_se_metrics
    assert SDR is BSSSDR and SDR is not PackageSDR and PackageSDR.KEYS == ("SI-SDR", "SNR", "SegSNR")
    assert fast_se_metrics.__all__ == ["STOI", "PESQ"]
    m = SDR(16000)
    assert m.higher_is_better and m.device == "cpu" and m.EXPECTED_SAMPLING_RATE == 16000
    assert (m.filter_length, m.zero_mean, m.load_diag) == (512, False, None) and SDR.KEYS == ("SDR",)
    c, n = bc.white_rows(3, 2000)
    res = m(c, n)
    assert isinstance(res, list) and len(res) == 3 and [tuple(r) for r in res] == [("SDR",)] * 3
    s = m.scores(c, n)
    assert s.dtype == torch.float32 and s.shape == (3,)
    assert [r["SDR"] for r in res] == [float(v) for v in s]
    with pytest.raises(Exception, match="should have the same shape"):
        m(c, n[:, :-1])
    with pytest.raises(Exception, match="should have the same shape"):
        m.scores(c, n[:2])


@pytest.mark.parametrize("kind", ["speech", "white"])
@pytest.mark.parametrize("scale", [1.0, 32768.0])
def test_cpu_mode_matches_definition(kind, scale):
    from fast_speech_enhancement_metrics_amd import BSSSDR, _cpu
    c, n = bc.speech_rows(4, 32000) if kind == "speech" else bc.white_rows(4, 32000)
    want, keep = bc.expected(c, n)
    c, n = c * scale, n * scale  # (exact: a power of two; the normalisation cancels it)
    ws, ks = bc.expected(c, n)
    assert keep.sum() >= 3 and ks.sum() >= 3
    both = keep & ks
    assert np.abs(want[both] - ws[both]).max() <= bc.ATOL_DB
    bc.assert_close(_cpu.bsssdr(c, n), ws, ks, f"_cpu.bsssdr {kind} x{scale:g}")
    m = BSSSDR(16000, use_gpu=False)
    bc.assert_close(m.scores(c, n), ws, ks, f"cpu scores {kind} x{scale:g}")
    bc.assert_close(m(c, n), ws, ks, f"cpu call {kind} x{scale:g}")


def test_cases_are_stable():
    """At most one case in eight is dropped because the definition's two evaluations (np.linalg.solve,
    the written-out Levinson recursion) disagree by more than 1e-4 dB; counted over the rows of the
    CPU and GPU tests' case sets."""
    sets = [bc.speech_rows(4, 32000), bc.white_rows(4, 32000), bc.delay_rows(), bc.edge_rows(),
            bc.speech_rows(4, 30001), bc.speech_rows(4, 16000, sr=8000)]
    keep = np.concatenate([bc.expected(c, n)[1] for c, n in sets])
    for name in GOLDEN_FILES:
        with np.load(os.path.join(bc.GOLDEN, f"{name}.npz")) as z:
            if int(z["sample_rate"]) == 16000:
                c, n = bc.golden(name)[:2]
                keep = np.concatenate([keep, bc.expected(c, n)[1]])
    print(f"{int((~keep).sum())} of {keep.size} cases dropped as unstable")
    assert 8 * int((~keep).sum()) <= keep.size


def test_golden_against_the_reference():
    """CPU mode against the reference's scores on the rows it could score alone (info == 0), at
    twice the reference's own largest distance from the definition, capped at 1e-2 dB; the rows on
    which the reference alone is further off are flagged and left out: at most one golden row in eight.
    Measured when the fixtures were made: bar 6.94e-3 dB; flagged: the 34.1 dB speech-like 16 kHz row
    (reference 1.26e-2 dB off) and the white row with noise at -50 dB (0.605 dB off), 2 of the 18 golden
    rows -- 2 of the 15 that carry a reference score, which would be above one in eight."""
    from fast_speech_enhancement_metrics_amd import BSSSDR
    bar = bc.golden_bar(*GOLDEN_FILES)
    print(f"bar against the reference: {bar:.3e} dB")
    assert 0 < bar <= bc.REF_CAP_DB
    rows = flagged = speech_scored = speech = 0
    for name in GOLDEN_FILES:
        c, n, sr, ref, has_ref, ref_ok = bc.golden(name)
        rows += len(ref)
        flagged += int((has_ref & ~ref_ok).sum())
        if name != "bsssdr_white":
            speech, speech_scored = speech + len(ref), speech_scored + int(has_ref.sum())
        else:
            assert has_ref[:4].all()  # every white row carries a reference score
        m = BSSSDR(sr, use_gpu=False)
        got = m(c, n)
        bc.assert_close(got, ref, ref_ok, f"cpu call vs reference {name}", atol=bar)
        c16, n16 = m.prepare_inputs(c, n)
        want, keep = bc.expected(c16, n16)
        bc.assert_close(got, want, keep, f"cpu call vs definition {name}")
    print(f"{flagged} of {rows} golden rows flagged: the reference is more than 1e-2 dB from the definition")
    assert 2 * speech_scored >= speech and 8 * flagged <= rows


def test_edge_semantics():
    from fast_speech_enhancement_metrics_amd import BSSSDR
    c, n = bc.edge_rows()
    want, keep = bc.expected(c, n)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = BSSSDR(16000, use_gpu=False).scores(c, n)
    bc.assert_close(got, want, keep, "cpu edges")
    g = got.double().numpy()
    assert g[0] >= 60 and g[3] >= 60 and g[0] <= 80.001 and g[3] <= 80.001  # identical rows, a gain
    assert g[1] == -80.0                                                    # a silent denoised row
    assert np.isnan(g[2]) and np.isfinite(g[[0, 1, 3, 4]]).all()            # a silent clean row, alone


def test_delays_inside_and_outside_the_filter():
    from fast_speech_enhancement_metrics_amd import BSSSDR
    c, n = bc.delay_rows()
    want, keep = bc.expected(c, n)
    assert keep.all() and want[0] > 15 and want[1] < 0
    bc.assert_close(BSSSDR(16000, use_gpu=False).scores(c, n), want, keep, "cpu delays")


def test_ragged_rows_and_no_samples():
    from fast_speech_enhancement_metrics_amd import BSSSDR
    lens = [0, 512, 513, 1023, 1024, 1025, 3000]
    c, n = bc.white_rows(len(lens), 3000, seed=13)
    want, keep = bc.expected(c, n, lens)
    assert np.isnan(want[0]) and keep.all()
    m = BSSSDR(16000, use_gpu=False)
    bc.assert_close(m.scores(c, n, lengths=lens), want, keep, "cpu ragged")
    res = m([c[b, :k] for b, k in enumerate(lens)], [n[b, :k] for b, k in enumerate(lens)])
    bc.assert_close(res, want, keep, "cpu ragged list")
    assert np.isnan(bc.values(m(c[:, :0], n[:, :0]))).all()
    # rows shorter than the filter: finite or NaN, and the same alone as in a batch
    short = m.scores(c, n, lengths=[1, 7, 100, 511, 300, 64, 2])
    for b, k in enumerate([1, 7, 100, 511, 300, 64, 2]):
        alone = m.scores(c[b:b + 1, :k], n[b:b + 1, :k])
        assert not torch.isinf(short[b]) and torch.equal(short[b:b + 1].isnan(), alone.isnan())
        assert torch.equal(short[b:b + 1].nan_to_num(), alone.nan_to_num())


def test_nonfinite_row_is_nan_alone():
    pm.nonfinite_row_is_nan_alone("BSSSDR")


def test_load_diag_and_fixed_attributes():
    from fast_speech_enhancement_metrics_amd import BSSSDR
    c, n = bc.white_rows(2, 4000)
    m = BSSSDR(16000)
    base = m.scores(c, n)
    m.load_diag = 0.5  # added to r[0] (= 1 after the normalisation): the filter explains less
    got = m.scores(c, n)
    r, b = bc.correlations(c[0].numpy(), n[0].numpy())
    r[0] += 0.5
    idx = np.abs(np.arange(512)[:, None] - np.arange(512)[None, :])
    coh = float(b @ np.linalg.solve(r[idx], b))
    assert abs(float(got[0]) - 10 * np.log10(coh / (1 - coh))) <= bc.ATOL_DB and (got < base).all()
    m.load_diag, m.zero_mean = None, True
    with pytest.raises(NotImplementedError):
        m.scores(c, n)


# ------------------------------------------------------------------ the C-ABI, host side
def test_abi_geometry(blib):
    assert blib.fsem_bsssdr_filter_length() == 512
    C, NC = blib.fsem_bsssdr_chunk(), blib.fsem_bsssdr_norm_chunk()
    assert C > 0 and C % 2048 == 0 and NC > 0 and NC % 256 == 0


def test_abi_validation_without_launch(blib):
    from fast_speech_enhancement_metrics_amd import _native
    ok, size = pm.one_output_validation(blib, "bsssdr")
    names = "ref deg batch length ld lengths load out ws ws_bytes"
    load_diag = contract.by_name(blib.fsem_bsssdr_load_diag_f32, names, None)
    contract.refusals(load_diag, dict(ok, load=0.0), [(dict(load=float("nan")), _native.FSEM_EINVAL),
                                                      (dict(ws_bytes=size - 1), _native.FSEM_EWORKSPACE)])
