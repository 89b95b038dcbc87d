"""SRMR on the HIP engine (csrc/srmr.hip) against the float64 statement of the definition
(tests/srmr_cases.py): frame and tile edges at both rates, mixed `lengths` with NaN planted past each
row, layouts, batch / position / stream invariance, the drop-in call and the NaN conventions.

The bars are a property of the statement, not of the engine: 4 x the largest relative
|complex64 statement - float64 statement| over the test's own rows (a chunked scan rounds in another
order than a sequential one, not in another kind)."""
import ctypes

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SRMR, _native

from . import srmr_cases as sc
from .contract import assert_bitwise, bits, on_side_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[8000, 16000])
def rows(request):
    """(rate, the edge rows with their statements, a metric, each row scored alone on the GPU)."""
    sr = request.param
    refs = sc.edge_rows(sr)
    m = SRMR(sr, use_gpu=True)
    alone = [m.scores(torch.from_numpy(x.copy()).cuda()[None], return_energies=True) for x, _, _ in refs]
    torch.cuda.synchronize()
    return sr, refs, m, alone


def padded(refs, idx, fill=float("nan"), extra=0):
    """The rows idx as one [B, L + extra] host batch, `fill` past each row's length."""
    lens = [len(refs[i][0]) for i in idx]
    x = torch.full((len(idx), max(lens) + extra), fill)
    for b, i in enumerate(idx):
        x[b, :lens[b]] = torch.from_numpy(refs[i][0].copy())
    return x, lens


def test_edge_shapes_alone_against_the_statement(rows):
    """B = 1 at n = wl - 1 (NaN), wl, wl + wi - 1, wl + wi, kT - 1, kT, kT + 1, kT + wi and 1.5 s."""
    sr, refs, m, alone = rows
    wi, wl = sc.geometry(sr)
    assert [len(r[0]) for r in refs][:4] == [wl - 1, wl, wl + wi - 1, wl + wi]
    assert [len(r[0]) for r in refs][4:7] == [2 * m.TILE - 1, 2 * m.TILE, 2 * m.TILE + 1]
    sbar, ebar = sc.bars(refs)
    print(f"gpu {sr}: score bar {sbar:.3e}, energy bar {ebar:.3e}")
    for (x, f64, c64), (s, A) in zip(refs, alone):
        assert s.is_cuda and s.dtype == torch.float32 and s.shape == (1,)
        assert A.is_cuda and A.dtype == torch.float64 and A.shape == (1, 23, 8)
        if not np.isfinite(f64[0]):
            assert torch.isnan(s).all() and torch.isnan(A).all() and len(x) == wl - 1
            continue
        ds = sc.rel(float(s[0]), f64[0])
        de = float(np.abs(A[0].cpu().numpy() - f64[1]).max() / f64[1].max())
        print(f"gpu {sr} n = {len(x)}: SRMR {float(s[0]):.6f} (statement {f64[0]:.6f}), relative {ds:.3e} "
              f"(complex64 statement {sc.rel(c64[0], f64[0]):.3e}); energies {de:.3e}")
        assert ds <= sbar, (len(x), float(s[0]), f64[0])
        assert de <= ebar, (len(x), de)


def test_mixed_lengths_with_nan_past_each_row(rows):
    """B = 5, NaN planted past every row's length: each row bitwise what it scores alone."""
    sr, refs, m, alone = rows
    idx = [8, 0, 5, 2, 7]
    x, lens = padded(refs, idx)
    s, A = m.scores(x.cuda(), lengths=lens, return_energies=True)
    assert s.shape == (5,) and A.shape == (5, 23, 8)
    for b, i in enumerate(idx):
        assert_bitwise((s[b:b + 1], A[b:b + 1]), alone[i], f"row {i} (n = {lens[b]}) at position {b} of 5")
    assert torch.isnan(s[1]) and torch.isfinite(s[[0, 2, 3, 4]]).all()
    # the same rows with a device int32 lengths tensor and a larger capacity
    xl, _ = padded(refs, idx, fill=3.0, extra=777)
    s2, A2 = m.scores(xl.cuda(), lengths=torch.tensor(lens, dtype=torch.int32, device="cuda"), return_energies=True)
    assert_bitwise((s2, A2), (s, A), "a larger row capacity")


def _call(lib, x, sr, lengths=None, stream=None):
    """fsem_srmr_f32 on device rows (any stride, any 4-byte alignment): (scores [B], energies [B, 23, 8])."""
    B, L = x.shape
    out = torch.full((B,), -7.0, device="cuda")
    A = torch.full((B, 23, 8), -7.0, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = lib.fsem_srmr_f32(p(x.data_ptr()), B, L, x.stride(0), p(lengths.data_ptr()) if lengths is not None else None,
                           sr, p(A.data_ptr()), p(out.data_ptr()), p(st))
    assert rc == _native.FSEM_OK, rc
    return out, A


def test_layouts_positions_and_streams(rows):
    sr, refs, m, alone = rows
    lib = _native.load()
    idx = [6, 3, 5]  # n = kT + 1 (odd), wl + wi, kT
    x, lens = padded(refs, idx, fill=0.5)
    L = x.shape[1]
    flat = torch.full((1 + 3 * (L + 3),), 9.0, device="cuda")
    strided = torch.as_strided(flat[1:], (3, L), (L + 3, 1))  # ld = L + 3 behind a base offset of 4 bytes
    assert strided.data_ptr() % 16 == 4 and strided.stride(0) == L + 3
    strided.copy_(x)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    got = m.scores(strided, lengths=lens_d, return_energies=True)
    for b, i in enumerate(idx):
        assert_bitwise((got[0][b:b + 1], got[1][b:b + 1]), alone[i], f"ld = L + 3, base + 4 bytes, row {i}")
    raw = _call(lib, strided, sr, lengths=lens_d)
    assert_bitwise(raw, got, "the C entry on the same rows")
    # another position and another batch size
    perm = [2, 0, 1]
    got_p = m.scores(x.cuda()[perm], lengths=[lens[j] for j in perm], return_energies=True)
    assert_bitwise(got_p, (got[0][perm], got[1][perm]), "rows permuted")
    # a side stream
    s_side = on_side_stream(lambda: m.scores(strided, lengths=lens_d, return_energies=True))
    assert_bitwise(s_side, got, "side stream")


def test_drop_in_call_lists_and_devices(rows):
    sr, refs, m, alone = rows
    idx = [1, 4, 0, 8]
    x, lens = padded(refs, idx, fill=0.0)
    xg = x.cuda()
    want = torch.cat([alone[i][0] for i in idx]).cpu().numpy()
    for res in (m(None, xg, lengths=lens), m(xg, xg, lengths=lens),
                m(None, [xg[b, :k] for b, k in enumerate(lens)])):
        assert [tuple(r) for r in res] == [("SRMR",)] * 4
        np.testing.assert_array_equal(np.array([r["SRMR"] for r in res], dtype=np.float32).view(np.uint32),
                                      want.view(np.uint32))
    with pytest.raises(Exception, match="same shape"):
        m(xg[:, :-1], xg)
    plain = m.scores(xg, lengths=lens)
    assert plain.shape == (4,) and plain.dtype == torch.float32
    np.testing.assert_array_equal(bits(plain), want.view(np.uint32))
    m2 = SRMR(sr, use_gpu=True, devices=[0, 0])
    np.testing.assert_array_equal(bits(m2.scores(xg, lengths=lens)), want.view(np.uint32))
    # the CPU mode agrees within the float32 bar
    cpu = SRMR(sr).scores(x[1:2, :lens[1]]).numpy()
    assert sc.rel(float(cpu[0]), float(want[1])) <= sc.bars(refs)[0] + 2.0 ** -23


def test_nan_rows_leave_their_neighbours_untouched(rows):
    sr, refs, m, alone = rows
    wi, wl = sc.geometry(sr)
    n = len(refs[3][0])  # wl + wi
    x = torch.from_numpy(np.stack([refs[3][0]] * 5).copy())
    x[1] = 0.0  # digitally silent: 0 / 0
    x[2, n - 1] = float("inf")
    x[3, 5] = float("nan")
    s, A = m.scores(x.cuda(), return_energies=True)
    assert torch.isnan(s[1:4]).all() and (A[1] == 0).all()
    for b in (0, 4):
        assert_bitwise((s[b:b + 1], A[b:b + 1]), alone[3], f"row {b} beside NaN rows")
    # rows too short for a frame, beside a scored one
    s, A = m.scores(x.cuda(), lengths=[n, wl - 1, 0, 1, n], return_energies=True)
    assert torch.isnan(s[1:4]).all() and torch.isnan(A[1:4]).all()
    for b in (0, 4):
        assert_bitwise((s[b:b + 1], A[b:b + 1]), alone[3], f"row {b} beside rows without a frame")


def test_abi_on_the_device():
    lib = _native.load()
    x = torch.zeros(4, 8000, device="cuda")
    o = torch.zeros(4, device="cuda")
    A = torch.zeros(4, 23, 8, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p
    for sr in (3999, 22050, 48000):
        assert lib.fsem_srmr_f32(p(x.data_ptr()), 4, 8000, 8000, None, sr, p(A.data_ptr()), p(o.data_ptr()), None) == \
            _native.FSEM_ERATE
    assert lib.fsem_srmr_f32(p(x.data_ptr()), 0, 8000, 8000, None, 8000, p(A.data_ptr()), p(o.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (o == 0).all() and (A == 0).all()  # batch == 0: nothing launched
    assert lib.fsem_srmr_f32(p(x.data_ptr()), 4, 0, 8000, None, 8000, p(A.data_ptr()), p(o.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and torch.isnan(A).all()  # length == 0: every score NaN
    assert lib.fsem_srmr_f32(p(x.data_ptr()), 4, 8000, 8000, None, 8000, p(A.data_ptr()), p(o.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and (A == 0).all()  # a silent batch: zero energies, 0 / 0
