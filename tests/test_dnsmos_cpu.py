"""DNSMOS metric without a GPU: the library's exports, build id and pinned workspace sizes, the weights
file, the segment rule, the CPU mode against the reference's float32 results (tests/golden/dnsmos_*.npz),
the interface (clean=None, shape check, 1-D input, lists and lengths=, the alias path, the weights
lookup) and the NaN rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import DNSMOS, _cpu

from . import contract
from . import dnsmos_cases as dc


@pytest.fixture(scope="module")
def dlib():
    """libfsem_dnsmos.so (include/fsem_dnsmos.h), built with libfsem.so."""
    from fast_speech_enhancement_metrics_amd import _build, _native
    _build.build()
    return _native.load_dnsmos()


@pytest.fixture(scope="module")
def metric():
    return DNSMOS(16000, use_gpu=False)


# ------------------------------------------------------------------ library and fixtures
def test_weights_file():
    from fast_speech_enhancement_metrics_amd.DNSMOS import WEIGHT_SHAPES, load_weights
    arrays = {}
    for p in (dc.WEIGHTS, dc.WEIGHTS[:-4] + "_2.npz"):
        assert os.path.getsize(p) < (1 << 20)
        with np.load(p, allow_pickle=False) as z:
            arrays.update({k: z[k] for k in z.files})
    assert len(arrays) == 22 and list(WEIGHT_SHAPES) != [] and set(arrays) == set(WEIGHT_SHAPES)
    for k, shape in WEIGHT_SHAPES.items():
        assert arrays[k].shape == shape and arrays[k].dtype == np.float32, k
    w = load_weights(dc.WEIGHTS)
    assert list(w) == list(WEIGHT_SHAPES) and all(t.dtype == torch.float32 for t in w.values())


def test_segment_counts(dlib):
    for n, want in dc.KNOWN_SEGMENTS.items():
        assert dc.segments_rule(n) == want
    for n in dc.SEGMENT_LENGTHS:
        want = dc.segments_rule(n)
        assert dlib.fsem_dnsmos_segments(n) == want == _cpu.dnsmos_segments(n), n
    assert dlib.fsem_dnsmos_segments(0) == 0 and dlib.fsem_dnsmos_segments(-5) == 0


def test_abi_validation_without_launch(dlib):
    from fast_speech_enhancement_metrics_amd import _native
    null, p = None, ctypes.c_void_p(256)
    big, over = 1 << 40, (1 << 29) + 4
    small = dlib.fsem_dnsmos_min_workspace_bytes()
    ok = dict(deg=p, batch=4, length=160000, ld=160000, lengths=null, blob=p, out=p, ws=p, ws_bytes=big)
    table = contract.nulled(_native.FSEM_EINVAL, "deg blob out") + contract.each(
        _native.FSEM_EINVAL, dict(batch=0), dict(length=0, ld=0), dict(ld=159999),
        dict(batch=1, length=over, ld=over, ws_bytes=1 << 62)) + contract.each(
        _native.FSEM_EWORKSPACE, dict(ws_bytes=small - 1), dict(ws_bytes=16), dict(ws=null))
    for f in (dlib.fsem_dnsmos_f32, dlib.fsem_dnsmos_features_f32, dlib.fsem_dnsmos_raw_f32):
        contract.refusals(contract.by_name(f, "deg batch length ld lengths blob out ws ws_bytes", null), ok, table)
    pack = dlib.fsem_dnsmos_pack_weights_f32
    ptrs = (ctypes.c_void_p * 22)(*([256] * 22))
    assert pack(None, p, big, null) == _native.FSEM_EINVAL and pack(ptrs, None, big, null) == _native.FSEM_EINVAL
    assert pack(ptrs, p, dlib.fsem_dnsmos_weights_bytes() - 1, null) == _native.FSEM_EWORKSPACE
    ptrs[7] = None
    assert pack(ptrs, p, big, null) == _native.FSEM_EINVAL


# ------------------------------------------------------------------ CPU-mode parity
@pytest.mark.parametrize("name", dc.FIXTURES)
def test_cpu_mode_matches_the_reference_in_float32(name):
    fx = dc.fixture(name)
    m = DNSMOS(fx.sample_rate, use_gpu=False)
    got = m.scores(fx.rows, sample_rate=fx.sample_rate)
    assert got.dtype == torch.float32 and got.shape == (fx.rows.shape[0], 3)
    # the 8 kHz rows pass through this package's resampler, the reference's through its own
    dc.assert_within(got, fx.ref32, dc.CPU_BAR, f"cpu scores {name}")
    if name == "dnsmos_short":  # the all-zero row and the quiet row: finite, where the reference's half precision is NaN
        assert np.isnan(fx.ref16[1:]).all() and torch.isfinite(got[1:]).all()
    if fx.sample_rate == 16000:
        raw = torch.cat([_cpu.dnsmos_raw(m.weights, r) for r in fx.rows])
        dc.assert_within(raw, fx.ref32_raw, dc.CPU_BAR, f"cpu raw outputs {name}")


# ------------------------------------------------------------------ interface
def test_interface(metric):
    fx = dc.fixture("dnsmos_short")
    x = fx.rows  # (40000-sample rows: one segment each)
    assert metric.higher_is_better and metric.EXPECTED_SAMPLING_RATE == 16000 and metric.device == "cpu"
    assert DNSMOS.KEYS == ("SIG", "BAK", "OVRL")
    res = metric(None, x)
    assert isinstance(res, list) and len(res) == 3 and [tuple(r) for r in res] == [DNSMOS.KEYS] * 3
    assert all(isinstance(v, float) for r in res for v in r.values())
    s = metric.scores(x)
    assert [[r[k] for k in DNSMOS.KEYS] for r in res] == [[float(v) for v in row] for row in s]
    with pytest.raises(Exception, match="`clean_speech` and `denoised_speech` should have the same shape."):
        metric(x[:, :-1], x)
    with pytest.raises(Exception, match="should have the same shape"):
        metric(x[:2], x)
    # 1-D input, with a clean row (which is only shape-checked)
    assert metric(x[0], x[0]) == res[:1]
    # lists and lengths= (19000 and 37000 samples double to one segment too)
    lens = [40000, 19000, 37000]
    ragged = metric(None, [x[b, :k] for b, k in enumerate(lens)])
    assert ragged[0] == res[0] and ragged[1] == res[1]  # (the full row; zeros score alike at any length)
    assert ragged[2] == metric(None, x[2, :37000])[0] != res[2]
    by_len = metric.scores(x, lengths=torch.tensor(lens))
    assert [[r[k] for k in DNSMOS.KEYS] for r in ragged] == [[float(v) for v in row] for row in by_len]


def test_alias_path_and_exports():
    import fast_se_metrics
    import fast_speech_enhancement_metrics_amd as pkg
    from fast_se_metrics.DNSMOS import DNSMOS as DropIn
    assert DropIn is DNSMOS and "DNSMOS" in pkg.__all__
    assert fast_se_metrics.__all__ == ["STOI", "PESQ"]


def test_weights_lookup(tmp_path, monkeypatch):
    from fast_speech_enhancement_metrics_amd.DNSMOS import DEFAULT_WEIGHTS, load_weights
    assert os.path.samefile(DEFAULT_WEIGHTS, dc.WEIGHTS)
    missing = str(tmp_path / "none.npz")
    with pytest.raises(FileNotFoundError, match=r"weights=.*FSEM_DNSMOS_WEIGHTS"):
        DNSMOS(16000, weights=missing)
    monkeypatch.setenv("FSEM_DNSMOS_WEIGHTS", missing)
    with pytest.raises(FileNotFoundError, match="none.npz"):
        DNSMOS(16000)
    # a state-dict .pt and a one-file .npz name the same weights
    w = load_weights(dc.WEIGHTS)
    pt, npz = str(tmp_path / "w.pt"), str(tmp_path / "one.npz")
    torch.save(w, pt)
    np.savez(npz, **{k: v.numpy() for k, v in w.items()})
    monkeypatch.setenv("FSEM_DNSMOS_WEIGHTS", pt)
    m = DNSMOS(16000)
    assert m.weights_file == pt and all(torch.equal(m.weights[k], w[k]) for k in w)
    m2 = DNSMOS(16000, weights=npz)
    assert all(torch.equal(m2.weights[k], w[k]) for k in w)
    np.savez(str(tmp_path / "short.npz"), **{k: v.numpy() for k, v in list(w.items())[:5]})
    with pytest.raises(ValueError, match="is missing"):
        DNSMOS(16000, weights=str(tmp_path / "short.npz"))


def test_nonfinite_and_empty_rows_are_nan_alone(metric):
    fx = dc.fixture("dnsmos_16k")
    x = fx.rows[:, :9500].clone()  # (9500 samples double to 152000: one segment)
    base = metric.scores(x)
    assert torch.isfinite(base).all()
    y = x.clone()
    y[0, 4000] = float("nan")
    y[2, 9499] = float("inf")
    got = metric.scores(y)
    assert torch.isnan(got[[0, 2]]).all() and torch.equal(got[1], base[1])
    res = metric(None, [x[0], x[1, :0], x[2]])
    assert all(np.isnan(v) for v in res[1].values()) and list(res[1]) == list(DNSMOS.KEYS)
    assert [res[b][k] for b in (0, 2) for k in DNSMOS.KEYS] == [float(v) for v in base[[0, 2]].reshape(-1)]
    assert torch.isnan(metric.scores(x[:, :0])).all()
