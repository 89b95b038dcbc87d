"""LSD metric on the HIP engine (csrc/lsd.hip) against the float64 statement of the definition
(tests/lsd_cases.py) and the reference's scores: parity, gain and edge rows, frame and chunk edges,
row layouts, streams, non-finite rows, the grid.y limit, devices= and the CPU mode."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import LSD, _native

from . import lsd_cases as lc

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_bitwise(got, want, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


@pytest.fixture(scope="module")
def rows16():
    """The 16 kHz parity rows (host), their float64 scores and a metric."""
    c, n = lc.speech_rows(4, 48000)
    return c, n, lc.expected(c, n), LSD(16000, use_gpu=True)


def test_parity_16k_and_int16_scale(rows16):
    c, n, want, m = rows16
    got = m.scores(c.cuda(), n.cuda())
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (4,)
    lc.assert_close(got, want, "gpu 16000")
    cs, ns = c * 32768, n * 32768  # (exact: powers of two)
    lc.assert_close(m.scores(cs.cuda(), ns.cuda()), lc.expected(cs, ns), "gpu 16000 x32768")


def test_golden_16k(rows16):
    c, n, sr, ref = lc.golden("lsd_16k")
    assert sr == 16000
    lc.assert_close(rows16[3](c.cuda(), n.cuda()), ref, "gpu call vs reference 16k", atol=0.0)


def test_golden_8k_resampled():
    c, n, sr, ref = lc.golden("lsd_8k")
    m = LSD(8000, use_gpu=True)
    cg, ng = c.cuda(), n.cuda()
    c16, n16 = m.prepare_inputs(cg, ng)
    assert c16.shape == (4, 48000)
    want = lc.expected(c16, n16)
    got = m(cg, ng)
    lc.assert_close(got, want, "gpu call 8k vs definition on the resampled rows")
    lc.assert_close(m.scores(cg, ng, sample_rate=8000), want, "gpu scores 8k")
    lc.assert_close(got, ref, "gpu call vs reference 8k", rtol=lc.RTOL_8K, atol=0.0)


def test_gain_cases(rows16):
    x, y = lc.gain_batch()
    lc.assert_close(rows16[3].scores(x.cuda(), y.cuda()), lc.expected(x, y), "gpu gain")


def test_edge_semantics(rows16):
    c, n = lc.edge_rows()
    m = rows16[3]
    got = m.scores(c.cuda(), n.cuda())
    lc.assert_close(got, lc.expected(c, n), "gpu edge rows")
    g = got.double().cpu().numpy()
    assert abs(g[0]) <= lc.ATOL
    assert abs(g[1] - lc.LN1E8) <= 1e-5 * lc.LN1E8 and abs(g[3] - lc.LN1E8) <= 1e-5 * lc.LN1E8
    assert np.isfinite(g[2]) and g[2] > 20
    assert abs(g[4]) <= lc.ATOL and abs(g[5]) <= lc.ATOL
    # n = 0 in a ragged list, and a batch of no samples
    lens = [0, 1, 255, 256, 700]
    c, n = lc.speech_rows(len(lens), 700, seed=13)
    res = m([c[b, :k].cuda() for b, k in enumerate(lens)], [n[b, :k].cuda() for b, k in enumerate(lens)])
    assert [tuple(r) for r in res] == [LSD.KEYS] * len(lens)
    lc.assert_close(res, lc.expected(c, n, lens), "gpu ragged list")
    lc.assert_close(m.scores(c[:, :0].cuda(), n[:, :0].cuda()), np.full(len(lens), lc.LN1E8), "gpu no samples")


def test_frame_and_chunk_edges(rows16):
    lib = _native.load_lsd()
    C = lib.fsem_lsd_chunk()
    cap = 2 * C + 257
    lens = [0, 1, 255, 256, 257, 511, 512, 513, C - 1, C, C + 1, C + 255, C + 256, 2 * C + 257]
    c, n = lc.speech_rows(len(lens), cap, seed=17)
    want = lc.expected(c, n, lens)
    # whatever the memory past a row's length holds
    cp, npad = c.clone(), n.clone()
    for b, k in enumerate(lens):
        cp[b, k:] = float("nan")
        npad[b, k:] = 1e30
    m = rows16[3]
    cg, ng = cp.cuda(), npad.cuda()
    got = m.scores(cg, ng, lengths=lens)
    lc.assert_close(got, want, "gpu frame and chunk edges")
    mask = torch.arange(cap)[None] < torch.tensor(lens)[:, None]
    cq = torch.where(mask, c, torch.tensor(1e30))
    nq = torch.where(mask, n, torch.tensor(float("nan")))
    assert_bitwise(m.scores(cq.cuda(), nq.cuda(), lengths=lens), got, "the padding swapped between the operands")
    for b, k in enumerate(lens):
        assert lib.fsem_lsd_frames(k) == 1 + k // 256
        if k == 0:
            continue  # (a batch needs a sample; the row's value is checked above)
        alone = m.scores(cg[b:b + 1, :k], ng[b:b + 1, :k])
        assert_bitwise(got[b:b + 1], alone, f"row {b} (n = {k}) alone")


def test_layouts(rows16):
    c, n, _, m = rows16
    L = 30001
    want = lc.expected(c[:, :L], n[:, :L])
    cg, ng = c.cuda(), n.cuda()
    base = m.scores(cg[:, :L].contiguous(), ng[:, :L].contiguous())  # L % 4 != 0
    lc.assert_close(base, want, "gpu L=30001")
    assert_bitwise(m.scores(cg[:, :L], ng[:, :L]), base, "strided view, L % 4 != 0")
    L4 = 30000
    want4 = lc.expected(c[:, :L4], n[:, :L4])
    v = m.scores(cg[:, :L4], ng[:, :L4])  # ld = 48000 > L, no copy
    lc.assert_close(v, want4, "gpu strided view")
    assert_bitwise(m.scores(cg[:, :L4].contiguous(), ng[:, :L4].contiguous()), v, "ld > L")
    # rows that do not start on 16-byte boundaries: the 4-byte loads give the same bits
    wide_c, wide_n = torch.zeros(4, 48003, device="cuda"), torch.zeros(4, 48003, device="cuda")
    wide_c[:, 1:L4 + 1], wide_n[:, 1:L4 + 1] = cg[:, :L4], ng[:, :L4]
    assert_bitwise(m.scores(wide_c[:, 1:L4 + 1], wide_n[:, 1:L4 + 1]), v, "unaligned rows")
    assert_bitwise(m.scores(cg[:, :L4].double(), ng[:, :L4].double()), v, "float64 input")
    ci, ni = (c[:, :L4] * 32768).round(), (n[:, :L4] * 32768).round()
    i16 = m.scores(ci.cuda().to(torch.int16), ni.cuda().to(torch.int16))
    lc.assert_close(i16, lc.expected(ci, ni), "gpu int16 input")
    assert_bitwise(i16, m.scores(ci.cuda(), ni.cuda()), "int16 input")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = m.scores(cg[:, :L], ng[:, :L])
    side.synchronize()
    assert_bitwise(s, base, "side stream")


def test_nonfinite_rows(rows16):
    c, n, want, m = rows16
    c2, n2 = c.clone(), n.clone()
    n2[1, 12345] = float("nan")
    c2[2, 47999] = float("inf")
    base, got = m.scores(c.cuda(), n.cuda()), m.scores(c2.cuda(), n2.cuda())
    assert torch.isnan(got[[1, 2]]).all()
    assert_bitwise(got[[0, 3]], base[[0, 3]], "finite rows beside non-finite ones")
    lc.assert_close(got, lc.expected(c2, n2), "gpu non-finite")


def test_past_grid_limit(rows16):
    NB = 65537
    c, n = lc.speech_rows(4, 600, seed=23)
    cg, ng = c.cuda(), n.cuda()
    m = rows16[3]
    small = m.scores(cg, ng)
    reps = -(-NB // 4)
    big = m.scores(cg.repeat(reps, 1)[:NB].contiguous(), ng.repeat(reps, 1)[:NB].contiguous())
    np.testing.assert_array_equal(_bits(big), _bits(small)[np.arange(NB) % 4])
    lc.assert_close(small, lc.expected(c, n), "gpu 600-sample rows")


def test_devices_fan_out(rows16):
    c, n, want, m = rows16
    m2 = LSD(16000, use_gpu=True, devices=[0, 0])
    cg, ng = c.cuda(), n.cuda()
    assert_bitwise(m2.scores(cg, ng), m.scores(cg, ng), "devices=[0, 0]")
    lens = [48000, 1000, 30001, 479]
    one = m.scores(cg, ng, lengths=lens)
    assert_bitwise(m2.scores(cg, ng, lengths=lens), one, "devices=[0, 0] with lengths")
    res = m2(cg, ng, lengths=lens)
    assert [tuple(r) for r in res] == [LSD.KEYS] * 4
    host = one.cpu().numpy()
    for b, r in enumerate(res):
        np.testing.assert_array_equal(np.float32(r["LSD"]), host[b])
    # copies and pickles drop what the metric keeps between calls (pinned buffers, the held list, the
    # fan-out's threads) and rebuild it on use
    for m3 in (copy.copy(m2), copy.deepcopy(m), pickle.loads(pickle.dumps(m2))):
        assert isinstance(m3, LSD) and m3.sample_rate == 16000
        assert_bitwise(m3.scores(cg, ng, lengths=lens), one, "a copied metric")
        assert m3(cg, ng, lengths=lens) == res


def test_cpu_mode_agrees(rows16):
    c, n, want, m = rows16
    cpu = LSD(16000, use_gpu=False).scores(c, n)
    lc.assert_close(cpu, want, "cpu 16000")
    lc.assert_close(m.scores(c.cuda(), n.cuda()), cpu.double().numpy(), "gpu vs cpu mode")


def test_abi_refuses_before_launch():
    lib = _native.load_lsd()
    x = torch.zeros(4, 1000, device="cuda")
    o = torch.zeros(4, device="cuda")
    p = ctypes.c_void_p
    args = (p(x.data_ptr()), p(x.data_ptr()), 4, 1000, 1000, None, p(o.data_ptr()))
    size = lib.fsem_lsd_workspace_bytes(4, 1000)
    ws = torch.zeros(size, dtype=torch.uint8, device="cuda")
    assert lib.fsem_lsd_f32(*args, p(ws.data_ptr()), 16, None) == _native.FSEM_EWORKSPACE
    assert lib.fsem_lsd_f32(*args, p(ws.data_ptr()), size - 1, None) == _native.FSEM_EWORKSPACE
    assert lib.fsem_lsd_f32(p(x.data_ptr()), p(x.data_ptr()), 4, 1000, 999, None, p(o.data_ptr()),
                            p(ws.data_ptr()), size, None) == _native.FSEM_EINVAL
    torch.cuda.synchronize()
    assert not o.any()  # (nothing ran)
