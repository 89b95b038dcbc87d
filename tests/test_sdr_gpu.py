"""SDR metric (SI-SDR, SNR, segmental SNR) on the HIP engine (csrc/sdr.hip) against the float64
statement of the definitions (tests/sdr_cases.py): parity at five rates, chunk and frame edges,
row layouts, streams, non-finite rows, the grid.y limit, devices= and the CPU mode."""
import ctypes
import math

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SDR, _native

from . import sdr_cases as sc

pytestmark = pytest.mark.gpu


def _bits(ts):
    return [t.cpu().numpy().view(np.uint32) for t in ts]


def assert_bitwise(got, want, what=""):
    for name, g, w in zip(SDR.KEYS, _bits(got), _bits(want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")


@pytest.fixture(scope="module")
def rows16():
    """The 16 kHz parity rows (host), their float64 scores and a metric."""
    c, n = sc.speech_rows(4, 48000, 16000, snr_high=40)
    return c, n, sc.expected(c, n, 16000), SDR(16000, use_gpu=True)


@pytest.mark.parametrize("sr,B,L", [(8000, 4, 24000), (22050, 4, 30000), (44100, 3, 50000), (48000, 3, 60000)])
def test_parity_rates(sr, B, L):
    c, n = sc.speech_rows(B, L, sr, snr_high=40)
    got = SDR(sr, use_gpu=True).scores(c.cuda(), n.cuda())
    assert all(g.is_cuda and g.dtype == torch.float32 and g.shape == (B,) for g in got)
    sc.assert_close(got, sc.expected(c, n, sr), f"gpu {sr}")


def test_parity_16k_and_int16_scale(rows16):
    c, n, want, m = rows16
    sc.assert_close(m.scores(c.cuda(), n.cuda()), want, "gpu 16000")
    cs, ns = c * 32768, n * 32768  # (exact: powers of two)
    sc.assert_close(m.scores(cs.cuda(), ns.cuda()), sc.expected(cs, ns, 16000), "gpu 16000 x32768")


def test_gain_cases(rows16):
    x, y = sc.gain_batch()
    sc.assert_close(rows16[3].scores(x.cuda(), y.cuda()), sc.expected(x, y, 16000), "gpu gain")


def test_zero_mean_dc_rows(rows16):
    c, n = rows16[0], rows16[1]
    cd, nd = sc.dc_rows(c, n)
    zm = SDR(16000, use_gpu=True, zero_mean=True)
    got = zm.scores(cd.cuda(), nd.cuda())
    sc.assert_close(got, sc.expected(cd, nd, 16000, zero_mean=True), "gpu zero_mean")
    free = sc.expected(c - c.mean(1, keepdim=True), n - n.mean(1, keepdim=True), 16000)
    np.testing.assert_allclose(got[0].cpu().numpy(), free[0], rtol=0, atol=sc.ATOL_SDR)
    off = rows16[3].scores(cd.cuda(), nd.cuda())
    assert_bitwise(got[1:], off[1:], "zero_mean leaves SNR / SegSNR")


@pytest.mark.parametrize("sr", [16000, 22050])
def test_chunk_and_frame_edges(sr):
    lib = _native.load()
    hop, win = sc.hop_win(sr)
    C = lib.fsem_sdr_chunk(sr)
    assert C % hop == 0 and hop == lib.fsem_sdr_hop(sr)
    cap = 2 * C + hop + 1
    lens = [0, 1, 3, win - 1, win, win + 1, win + hop - 1, win + hop,
            C - 1, C, C + 1, C + win - 1, C + win, 2 * C + hop + 1, cap]
    c, n = sc.speech_rows(len(lens), cap, sr, seed=17, snr_high=40)
    m = SDR(sr, use_gpu=True)
    cg, ng = c.cuda(), n.cuda()
    got = m.scores(cg, ng, lengths=lens)
    sc.assert_close(got, sc.expected(c, n, sr, lengths=lens), f"gpu edges {sr}")
    for b, k in enumerate(lens):
        assert lib.fsem_sdr_frames(k, sr) == ((k - win) // hop + 1 if k >= win else 0)
        if k == 0:
            continue  # (a batch needs a sample; the row's NaNs are checked above)
        alone = m.scores(cg[b:b + 1, :k], ng[b:b + 1, :k])
        assert_bitwise([g[b:b + 1] for g in got], alone, f"row {b} (n = {k}) alone")


def test_layouts(rows16):
    c, n, _, m = rows16
    L = 30001
    want = sc.expected(c[:, :L], n[:, :L], 16000)
    cg, ng = c.cuda(), n.cuda()
    base = m.scores(cg[:, :L].contiguous(), ng[:, :L].contiguous())  # L % 4 != 0
    sc.assert_close(base, want, "gpu L=30001")
    sc.assert_close(m.scores(cg[:, :L], ng[:, :L]), want, "gpu strided view, L % 4 != 0")
    L4 = 30000
    want4 = sc.expected(c[:, :L4], n[:, :L4], 16000)
    v = m.scores(cg[:, :L4], ng[:, :L4])  # ld = 48000 > L, no copy
    sc.assert_close(v, want4, "gpu strided view")
    # rows that do not start on 16-byte boundaries: the 4-byte loads give the same bits
    wide_c, wide_n = torch.zeros(4, 48003, device="cuda"), torch.zeros(4, 48003, device="cuda")
    wide_c[:, 1:L4 + 1], wide_n[:, 1:L4 + 1] = cg[:, :L4], ng[:, :L4]
    assert_bitwise(m.scores(wide_c[:, 1:L4 + 1], wide_n[:, 1:L4 + 1]), v, "unaligned rows")
    sc.assert_close(m.scores(cg[:, :L4].double(), ng[:, :L4].double()), want4, "gpu float64 input")
    ci, ni = (c[:, :L4] * 32768).round(), (n[:, :L4] * 32768).round()
    sc.assert_close(m.scores(ci.cuda().to(torch.int16), ni.cuda().to(torch.int16)), sc.expected(ci, ni, 16000),
                    "gpu int16 input")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = m.scores(cg[:, :L], ng[:, :L])
    side.synchronize()
    assert_bitwise(s, base, "side stream")


def test_nonfinite_rows(rows16):
    c, n, _, m = rows16
    c2, n2 = c.clone(), n.clone()
    n2[1, 12345] = float("nan")
    c2[2, 47999] = float("inf")
    base, got = m.scores(c.cuda(), n.cuda()), m.scores(c2.cuda(), n2.cuda())
    for b, g in zip(base, got):
        assert torch.isnan(g[[1, 2]]).all()
    assert_bitwise([g[[0, 3]] for g in got], [b[[0, 3]] for b in base], "finite rows beside non-finite ones")


def test_edge_semantics(rows16):
    c, n = sc.edge_rows()
    si, snr, seg = (v.cpu().numpy() for v in rows16[3].scores(c.cuda(), n.cuda()))
    sc.assert_close((si, snr, seg), sc.expected(c, n, 16000), "gpu edge semantics")
    assert si[0] == math.inf and snr[0] == math.inf and seg[0] == 35.0
    assert math.isnan(si[1]) and snr[1] == -math.inf and seg[1] == -10.0
    assert math.isnan(si[2]) and abs(snr[2]) < 1e-6
    assert math.isnan(si[3]) and math.isnan(snr[3]) and seg[3] == -10.0
    hop, win = sc.hop_win(16000)
    lens = [0, 1, win - 1, win, win + hop - 1, win + hop]
    c, n = sc.speech_rows(len(lens), win + hop, 16000, seed=13)
    res = rows16[3]([c[b, :k].cuda() for b, k in enumerate(lens)], [n[b, :k].cuda() for b, k in enumerate(lens)])
    assert [list(r) for r in res] == [["SI-SDR", "SNR", "SegSNR"]] * len(lens)
    sc.assert_close(np.array([[r[k] for r in res] for k in SDR.KEYS]), sc.expected(c, n, 16000, lengths=lens),
                    "gpu short list")


def test_past_grid_limit(rows16):
    NB = 65537
    c, n = sc.speech_rows(4, 600, 16000, seed=23)
    cg, ng = c.cuda(), n.cuda()
    m = rows16[3]
    small = m.scores(cg, ng)
    reps = -(-NB // 4)
    big = m.scores(cg.repeat(reps, 1)[:NB].contiguous(), ng.repeat(reps, 1)[:NB].contiguous())
    src = np.arange(NB) % 4
    for g, w in zip(_bits(big), _bits(small)):
        np.testing.assert_array_equal(g, w[src])
    sc.assert_close(small, sc.expected(c, n, 16000), "gpu 600-sample rows")


def test_devices_fan_out(rows16):
    c, n, want, m = rows16
    m2 = SDR(16000, use_gpu=True, devices=[0, 0])
    cg, ng = c.cuda(), n.cuda()
    assert_bitwise(m2.scores(cg, ng), m.scores(cg, ng), "devices=[0, 0]")
    lens = [48000, 1000, 30001, 479]
    one = m.scores(cg, ng, lengths=lens)
    assert_bitwise(m2.scores(cg, ng, lengths=lens), one, "devices=[0, 0] with lengths")
    res = m2(cg, ng, lengths=lens)
    assert [tuple(r) for r in res] == [SDR.KEYS] * 4
    host = [v.cpu().numpy() for v in one]
    for b, r in enumerate(res):
        for k, key in enumerate(SDR.KEYS):
            np.testing.assert_array_equal(np.float32(r[key]), host[k][b])


def test_cpu_mode_agrees(rows16):
    c, n, want, m = rows16
    cpu = SDR(16000, use_gpu=False).scores(c, n)
    sc.assert_close(cpu, want, "cpu 16000")
    sc.assert_close(m.scores(c.cuda(), n.cuda()), np.stack([v.double().numpy() for v in cpu]), "gpu vs cpu mode")


def test_abi_refuses_before_launch():
    lib = _native.load()
    x = torch.zeros(4, 1000, device="cuda")
    o = torch.zeros(3, 4, device="cuda")
    p = ctypes.c_void_p
    args = (p(x.data_ptr()), p(x.data_ptr()), 4, 1000, 1000, None)
    outs = (p(o[0].data_ptr()), p(o[1].data_ptr()), p(o[2].data_ptr()))
    assert lib.fsem_sdr_f32(*args, 3999, 0, *outs, p(x.data_ptr()), 1 << 20, None) == _native.FSEM_ERATE
    assert lib.fsem_sdr_f32(*args, 16000, 0, *outs, p(x.data_ptr()), 16, None) == _native.FSEM_EWORKSPACE
    torch.cuda.synchronize()
