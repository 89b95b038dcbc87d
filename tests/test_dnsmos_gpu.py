"""DNSMOS metric on the HIP engine (csrc/dnsmos.hip) against the reference's float32 results
(tests/golden/dnsmos_*.npz): score and raw-output parity, the feature stage, doubling and segment edges,
bitwise invariance (batch, position, padding, ld, alignment, workspace size, stream), non-finite and
empty rows, the 8 kHz path, the drop-in call and the C-ABI's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import DNSMOS, _native

from . import dnsmos_cases as dc
from .contract import assert_bitwise, on_side_stream

pytestmark = pytest.mark.gpu

# Rows that are not a fixture's own rows (cut, padded or repeated ones) are held to twice the largest
# stored basis: the basis is a sample of the f16 rounding noise of the network, and no row of the
# fixtures showed more.
SCORE_BAR = 2 * max(dc.fixture(n).basis for n in dc.FIXTURES)


@pytest.fixture(scope="module")
def metric():
    return DNSMOS(16000, use_gpu=True)


@pytest.fixture(scope="module")
def cpu_metric():
    return DNSMOS(16000, use_gpu=False)


def engine(entry: str, m, rows: torch.Tensor, lengths, cols, ws_bytes=None):
    """One direct call of a C-ABI entry on CUDA rows [B, L] (any row stride): the output as
    [S_total or B, *cols] float32."""
    lib = _native.load_dnsmos()
    B, L = rows.shape
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=rows.device)
    counts = [lib.fsem_dnsmos_segments(int(k)) for k in (lengths if lengths is not None else [L] * B)]
    n_out = B if entry == "fsem_dnsmos_f32" else sum(counts)
    out = torch.full((n_out, *cols), -7.0, dtype=torch.float32, device=rows.device)
    size = lib.fsem_dnsmos_workspace_bytes(B, L) if ws_bytes is None else ws_bytes
    ws = torch.empty(size, dtype=torch.uint8, device=rows.device)
    rc = getattr(lib, entry)(rows.data_ptr(), B, L, rows.stride(0), lens.data_ptr() if lens is not None else None,
                             m.blob(rows.device).data_ptr(), out.data_ptr(), ws.data_ptr(), size,
                             _native.stream_handle(rows.device))
    assert rc == _native.FSEM_OK, rc
    return out


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", dc.FIXTURES)
def test_scores_and_raw_outputs_match_the_reference_in_float32(name):
    fx = dc.fixture(name)
    m = DNSMOS(fx.sample_rate, use_gpu=True)
    x = fx.rows.cuda()
    got = m.scores(x, sample_rate=fx.sample_rate)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (x.shape[0], 3)
    print(f"{name}: ref16 NaN rows {np.isnan(fx.ref16).any(axis=1).tolist()}, basis {fx.basis:.3e} / {fx.basis_raw:.3e}")
    rows16, _ = m._engine_rows(x, fx.sample_rate, None)  # (the 8 kHz rows through the resampler)
    raw = engine("fsem_dnsmos_raw_f32", m, rows16, None, (3,))
    # no row skipped: the rows on which the reference's half precision is NaN are finite and inside the bar
    dc.assert_within(got, fx.ref32, 2 * fx.basis, f"gpu scores {name}")
    dc.assert_within(raw, fx.ref32_raw, 2 * fx.basis_raw, f"gpu raw outputs {name}")
    assert_bitwise(m.scores(x, sample_rate=fx.sample_rate), got, "a second call")


def test_feature_stage(metric):
    fx = dc.fixture("dnsmos_16k")
    rows = torch.cat([fx.rows, torch.zeros(1, dc.SEG)])
    got = engine("fsem_dnsmos_features_f32", metric, rows.cuda(), None, (900, 161)).cpu().double()
    want = dc.features64(metric.weights, rows, torch.float64)
    f32 = dc.features64(metric.weights, rows, torch.float32).double()
    bar = 4 * float((f32 - want).abs().max())
    err = float((got - want).abs().max())
    print(f"features: worst |engine - float64| = {err:.3e}; float32 torch against float64 {bar / 4:.3e} (bar {bar:.3e})")
    assert torch.isfinite(got).all() and err <= bar
    assert bool((got[3] == -12.0).all())  # the silent row: exactly -12 everywhere


# ------------------------------------------------------------------ doubling and segment edges
@pytest.mark.parametrize("n", [1, 319, 40000, 144159, 144160, 160159, 160160])
def test_doubling_and_segment_edges(metric, cpu_metric, n):
    row = dc.fixture("dnsmos_long").rows[0]
    lib = _native.load_dnsmos()
    assert lib.fsem_dnsmos_segments(n) == dc.segments_rule(n)
    x = row[500:500 + n].reshape(1, n)
    want = cpu_metric.scores(x)
    got = metric.scores(x.cuda())
    dc.assert_within(got, want.double().numpy(), SCORE_BAR, f"gpu vs cpu mode, {n} samples")
    raw = engine("fsem_dnsmos_raw_f32", metric, x.cuda(), None, (3,))
    assert raw.shape[0] == dc.segments_rule(n) and torch.isfinite(raw).all()


# ------------------------------------------------------------------ bitwise invariance and chunking
RAGGED = (40000, 177000, 144160, 1)  # 1 + 3 + 1 + 8 segments


@pytest.fixture(scope="module")
def ragged(metric):
    """A padded batch whose padding holds NaN, its scores, and each row's scores alone."""
    long = dc.fixture("dnsmos_long").rows[0]
    k16 = dc.fixture("dnsmos_16k").rows
    src = [k16[0], long, k16[1], k16[2]]
    pad = torch.full((4, 177000), float("nan"))
    for b, n in enumerate(RAGGED):
        pad[b, :n] = src[b][:n]
    got = metric.scores(pad.cuda(), lengths=list(RAGGED))
    return pad, got


def test_rows_score_as_the_row_alone(metric, ragged):
    pad, got = ragged
    assert torch.isfinite(got).all()
    g = pad.cuda()
    for b, n in enumerate(RAGGED):
        assert_bitwise(metric.scores(g[b:b + 1, :n].contiguous()), got[b:b + 1], f"row {b} ({n} samples) alone")
    # an odd row stride and a base pointer 4 bytes off a 16-byte boundary
    ld = 177001
    flat = torch.full((4 * ld + 8,), float("nan"), device="cuda")
    view = flat[1:1 + 4 * ld].view(4, ld)[:, :177000]
    view.copy_(g)
    assert view.data_ptr() % 16 == 4 and view.stride(0) == ld
    assert_bitwise(metric.scores(view, lengths=list(RAGGED)), got, "odd ld, offset base")
    s = on_side_stream(lambda: metric.scores(g, lengths=list(RAGGED)))
    assert_bitwise(s, got, "side stream")


def test_every_workspace_size_gives_the_same_bits(metric, ragged):
    pad, got = ragged
    lib = _native.load_dnsmos()
    small = lib.fsem_dnsmos_min_workspace_bytes()
    g = pad.cuda()
    assert sum(dc.segments_rule(n) for n in RAGGED) >= 12
    full = engine("fsem_dnsmos_f32", metric, g, list(RAGGED), (3,))
    assert_bitwise(full, got, "the recommended workspace")
    # one segment per pass, and two (2 * min holds two segments' buffers and not three): a pass
    # boundary falls inside the three-segment row and inside the eight-segment row
    assert_bitwise(engine("fsem_dnsmos_f32", metric, g, list(RAGGED), (3,), ws_bytes=small), got, "minimum workspace")
    assert_bitwise(engine("fsem_dnsmos_f32", metric, g, list(RAGGED), (3,), ws_bytes=2 * small), got,
                   "two segments per pass")
    raw = engine("fsem_dnsmos_raw_f32", metric, g, list(RAGGED), (3,))
    assert_bitwise(engine("fsem_dnsmos_raw_f32", metric, g, list(RAGGED), (3,), ws_bytes=small), raw, "raw, minimum")


# ------------------------------------------------------------------ non-finite and empty rows
def test_nonfinite_and_empty_rows(metric):
    x = dc.fixture("dnsmos_16k").rows[:, :9500].cuda()  # (9500 samples double to 152000: one segment)
    base = metric.scores(x)
    assert torch.isfinite(base).all()
    y = x.clone()
    y[0, 4000] = float("nan")
    y[2, 9499] = float("inf")
    got = metric.scores(y)
    assert torch.isnan(got[[0, 2]]).all()
    assert_bitwise(got[1:2], base[1:2], "the finite row between non-finite ones")
    got = metric.scores(x, lengths=[9500, 0, 9500])
    assert torch.isnan(got[1]).all()
    assert_bitwise(got[[0, 2]], base[[0, 2]], "rows beside an empty row")
    assert torch.isnan(metric.scores(x[:, :0])).all()
    res = metric(None, [x[0], x[1, :0]])
    assert all(np.isnan(v) for v in res[1].values()) and list(res[1]) == list(DNSMOS.KEYS)


# ------------------------------------------------------------------ the drop-in call, devices=, errors
def test_drop_in_call_on_a_side_stream(metric):
    x = dc.fixture("dnsmos_short").rows.cuda()
    want = metric.scores(x).cpu()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = metric(None, x)
        res2 = metric(x, x)
    assert isinstance(res, list) and [tuple(r) for r in res] == [DNSMOS.KEYS] * 3 and res == res2
    assert all(isinstance(v, float) for r in res for v in r.values())
    for b, r in enumerate(res):
        np.testing.assert_array_equal(np.float32([r[k] for k in DNSMOS.KEYS]), want[b].numpy())
    with pytest.raises(Exception, match="should have the same shape"):
        metric(x[:, :-1], x)
    m2 = DNSMOS(16000, use_gpu=True, devices=[0, 0])
    assert_bitwise(m2.scores(x), want, "devices=[0, 0]")
    assert m2(None, x) == res
    # copies and pickles drop the packed weights (per-device state) and rebuild them on use
    import copy
    import pickle
    for m3 in (copy.deepcopy(metric), pickle.loads(pickle.dumps(m2))):
        assert m3._blobs == {}
        assert_bitwise(m3.scores(x), want, "a copied metric")


def test_abi_refuses_before_launch(metric):
    lib = _native.load_dnsmos()
    x = torch.zeros(2, 40000, device="cuda")
    o = torch.zeros(2, 3, device="cuda")
    p = ctypes.c_void_p
    blob = metric.blob(x.device)
    small = lib.fsem_dnsmos_min_workspace_bytes()
    ws = torch.zeros(small, dtype=torch.uint8, device="cuda")
    f = lib.fsem_dnsmos_f32
    ok = (p(x.data_ptr()), 2, 40000, 40000, None, p(blob.data_ptr()), p(o.data_ptr()), p(ws.data_ptr()), small, None)

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)

    assert call(a0=None) == call(a5=None) == call(a6=None) == _native.FSEM_EINVAL
    assert call(a1=0) == call(a2=0) == call(a3=39999) == _native.FSEM_EINVAL
    assert call(a8=small - 1) == call(a8=16) == call(a7=None) == _native.FSEM_EWORKSPACE
    torch.cuda.synchronize()
    assert not o.any()  # (nothing ran)
