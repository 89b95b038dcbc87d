"""SpectralMeasures (fwSegSNR, CD, IS) on the HIP engine (csrc/spectral.hip) against the float64
statement of the definitions (tests/spectral_cases.py): parity at both rates, frame and group
edges, a long row through the radix select, a level gap, silent frames, non-finite rows, layouts,
`lengths`, batch and position invariance, the documented reduction, devices= and the CPU mode."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd import SpectralMeasures, _native

from . import sdr_cases as sc
from . import spectral_cases as sp
from . import contract
from . import pair_metrics as pm

pytestmark = pytest.mark.gpu
KEYS = SpectralMeasures.KEYS
assert_bitwise = functools.partial(contract.assert_bitwise, names=KEYS + ("frames",))


@pytest.fixture(scope="module", params=[8000, 16000])
def rows(request):
    """The parity rows of one rate (host), their float64 scores and a metric."""
    sr = request.param
    c, n = sp.parity_rows(sr)
    return sr, c, n, sp.expected(c, n, sr), SpectralMeasures(sr, use_gpu=True)


def test_parity_and_int16_scale(rows):
    sr, c, n, want, m = rows
    got = m.scores(c.cuda(), n.cuda())
    assert len(got) == 3 and all(g.is_cuda and g.dtype == torch.float32 and g.shape == (4,) for g in got)
    sp.assert_scores(got, c, n, sr, what=f"gpu {sr}", want=want)
    assert np.isfinite(sp.to_np(got)).all()
    cs, ns = c * 32768, n * 32768  # (exact: powers of two)
    sp.assert_scores(m.scores(cs.cuda(), ns.cuda()), cs, ns, sr, what=f"gpu {sr} x32768")


def test_frame_and_group_edges_and_lengths(rows):
    """n = win - 1, win, win + hop - 1, and F = GROUP - 1, GROUP, GROUP + 1, 2 GROUP + 1 (a block of
    the frame kernel takes GROUP frames, its last step one lane per frame and signal of them); every
    row with `lengths` bitwise what the row alone gives, frames included."""
    sr, m = rows[0], rows[4]
    c, n, lens = sp.edge_rows(sr)
    cg, ng = c.cuda(), n.cuda()
    got = m.scores(cg, ng, lengths=lens, return_frames=True)
    sp.assert_scores(got, c, n, sr, lengths=lens, what=f"gpu edges {sr}", atol=sp.ATOL_EDGE)
    assert got[3].shape == (3, len(lens), sp.frames_of(max(lens), sr))
    for b, k in enumerate(lens):
        F = sp.frames_of(k, sr)
        assert torch.isnan(got[3][:, b, F:]).all()  # (left unwritten by the engine: the class's NaN fill)
        if k == 0:
            continue  # (a batch needs a sample; the row's NaNs are checked above)
        alone = m.scores(cg[b:b + 1, :k], ng[b:b + 1, :k], return_frames=True)
        assert_bitwise([g[b:b + 1] for g in got[:3]] + [got[3][:, b:b + 1, :F]], alone, f"row {b} (n = {k}) alone")


def test_long_row_through_the_select(rows):
    """A row of about 8000 frames: 40 hops of speech repeated, so the frame values repeat with period
    40 (exact ties at the K-th value) and the float64 side stays small; the scores are also the
    documented reduction of the returned frames, bit for bit."""
    sr, m = rows[0], rows[4]
    hop, win = sc.hop_win(sr)
    period, reps = 40, 200
    c, n = sc.speech_rows(1, period * hop, sr, seed=29, snr_high=20)
    cl, nl = c.repeat(1, reps), n.repeat(1, reps)
    F = sp.frames_of(cl.shape[1], sr)
    assert F == period * reps - 3
    vals = sp.frame_values(cl[0, :period * hop + win - hop].numpy(), nl[0, :period * hop + win - hop].numpy(), sr)
    assert len(vals[0]) == period
    idx = np.arange(F) % period
    want = np.array(sp.row_values(*(v[idx] for v in vals)))[:, None]
    got = m.scores(cl.cuda(), nl.cuda(), return_frames=True)
    sp.assert_scores(got, cl, nl, sr, what=f"gpu long row {sr} ({F} frames)", want=want)
    fr = got[3].cpu().numpy()
    for k in range(3):
        np.testing.assert_array_equal(fr[k, 0, :F - period].view(np.uint32), fr[k, 0, period:].view(np.uint32))
        red = sp.engine_reduction(fr[k, 0], trimmed=k > 0)
        assert red.view(np.uint32) == got[k].cpu().numpy().view(np.uint32)[0], (KEYS[k], red, got[k])


def test_level_gap(rows):
    """s^ = 1e-5 (s + noise): fwSegSNR (normalised magnitudes) and CD (the cepstrum without c[0]) do
    not see the level; IS does, and follows the float64 definition (here: its clamp)."""
    sr, m = rows[0], rows[4]
    c, n, scaled = sp.level_gap_rows(sr)
    plain = m.scores(c.cuda(), n.cuda())
    gap = m.scores(c.cuda(), scaled.cuda())
    sp.assert_scores(plain, c, n, sr, what=f"gpu level gap {sr}, unscaled")
    sp.assert_scores(gap, c, scaled, sr, what=f"gpu level gap {sr}, scaled")
    p, g = sp.to_np(plain), sp.to_np(gap)
    for k in (0, 1):
        err = float(np.abs(p[k] - g[k]).max())
        print(f"gpu level gap {sr} {KEYS[k]}: worst |scaled - unscaled| = {err:.3e}")
        assert err <= sp.ATOL[KEYS[k]], (KEYS[k], p[k], g[k])


def test_silent_frames(rows):
    sr, m = rows[0], rows[4]
    hop, win = sc.hop_win(sr)
    c, n = sp.silent_head_rows(sr, win + 2 * hop)  # frames 0 .. 2 are silent in the clean row
    F = sp.frames_of(c.shape[1], sr)
    assert F - sp.trimmed_count(F) >= 3
    got = m.scores(c.cuda(), n.cuda(), return_frames=True)
    want = sp.assert_scores(got, c, n, sr, what=f"gpu silent clean head {sr}")
    assert np.isnan(want[0, 0]) and np.isfinite(want[1:, 0]).all()  # fwSegSNR NaN; CD, IS by the K rule
    fr = got[3].cpu().numpy()
    assert np.isnan(fr[:, 0, :3]).all() and np.isfinite(fr[:, 0, 3:]).all()
    # more silent frames than the trim takes away: CD and IS are NaN as well
    c2 = c.clone()
    c2[0, :win + 9 * hop] = 0
    got = m.scores(c2.cuda(), n.cuda())
    assert all(torch.isnan(g).all() for g in got)
    sp.assert_scores(got, c2, n, sr, what=f"gpu long silent clean head {sr}")
    # a silent denoised frame: fwSegSNR_f = 0 exactly (CD_f and IS_f NaN)
    n3 = n.clone()
    n3[0, :win] = 0
    fr = m.scores(n.cuda(), n3.cuda(), return_frames=True)[3].cpu().numpy()
    assert fr[0, 0, 0] == 0.0 and np.isnan(fr[1:, 0, 0]).all() and np.isfinite(fr[:, 0, 4:]).all()


def test_nonfinite_rows(rows):
    pm.nonfinite_rows(f"Spectral-{rows[0]}")


def _call(lib, c, n, sr, ldf=None, lengths=None):
    """fsem_spectral_f32 on device rows with one stride: (scores [3, B], frames [3, B, ldf])."""
    B, L = c.shape
    F = sp.frames_of(L, sr)
    ldf = max(F, 1) if ldf is None else ldf
    out = torch.full((3, B), -7.0, device="cuda")
    frames = torch.full((3, B, ldf), -7.0, device="cuda")
    p = ctypes.c_void_p
    rc = lib.fsem_spectral_f32(p(c.data_ptr()), p(n.data_ptr()), B, L, c.stride(0),
                               p(lengths.data_ptr()) if lengths is not None else None, sr, p(frames.data_ptr()), ldf,
                               *(p(out[k].data_ptr()) for k in range(3)), p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FSEM_OK, rc
    return out, frames


def test_layouts(rows):
    sr, c, n, _, m = rows
    lib = _native.load()
    L = c.shape[1] - 403  # odd: rows of a view start at any 4-byte boundary
    F = sp.frames_of(L, sr)
    cg, ng = c.cuda(), n.cuda()
    base = m.scores(cg[:, :L].contiguous(), ng[:, :L].contiguous(), return_frames=True)
    sp.assert_scores(base, c[:, :L], n[:, :L], sr, what=f"gpu {sr} odd length")
    assert_bitwise(m.scores(cg[:, :L], ng[:, :L], return_frames=True), base, "ld > length (views, no copy)")
    wide_c = torch.zeros(4, c.shape[1] + 3, device="cuda")
    wide_n = torch.zeros(4, c.shape[1] + 3, device="cuda")
    wide_c[:, 1:L + 1], wide_n[:, 1:L + 1] = cg[:, :L], ng[:, :L]
    assert wide_c[:, 1:].data_ptr() % 16 == 4 and wide_c.stride(0) % 4
    assert_bitwise(m.scores(wide_c[:, 1:L + 1], wide_n[:, 1:L + 1], return_frames=True), base, "unaligned rows")
    out, frames = _call(lib, wide_c[:, 1:L + 1], wide_n[:, 1:L + 1], sr, ldf=F + 5)
    assert_bitwise(list(out) + [frames[:, :, :F]], base, "ldf > F")
    assert (frames[:, :, F:] == -7.0).all()  # nothing written past the frames
    s = contract.on_side_stream(lambda: m.scores(cg[:, :L], ng[:, :L], return_frames=True))
    assert_bitwise(s, base, "side stream")


def test_batch_and_position_invariance(rows):
    sr, c, n, _, m = rows
    cg, ng = c.cuda(), n.cuda()
    base = m.scores(cg, ng, return_frames=True)
    perm = [2, 0, 3, 1]
    got = m.scores(cg[perm], ng[perm], return_frames=True)
    assert_bitwise(got, [b[perm] for b in base[:3]] + [base[3][:, perm]], "rows permuted")
    big = m.scores(cg.repeat(3, 1)[:7], ng.repeat(3, 1)[:7], return_frames=True)  # B = 7
    idx = [i % 4 for i in range(7)]
    assert_bitwise(big, [b[idx] for b in base[:3]] + [base[3][:, idx]], "batch of 7")
    # a longer capacity (`length`) with the same rows behind `lengths`
    L = c.shape[1]
    pad_c, pad_n = torch.nn.functional.pad(cg, (0, 777), value=1.0), torch.nn.functional.pad(ng, (0, 777), value=2.0)
    got = m.scores(pad_c, pad_n, lengths=[L] * 4, return_frames=True)
    F = sp.frames_of(L, sr)
    assert_bitwise(list(got[:3]) + [got[3][:, :, :F]], base, "a larger row capacity")


def test_scores_are_the_documented_reduction_of_the_frames(rows):
    sr, m = rows[0], rows[4]
    c, n, lens = sp.edge_rows(sr)
    got = m.scores(c.cuda(), n.cuda(), lengths=lens, return_frames=True)
    fr = got[3].cpu().numpy()
    for b, k in enumerate(lens):
        F = sp.frames_of(k, sr)
        for j in range(3):
            red = sp.engine_reduction(fr[j, b, :F], trimmed=j > 0)
            have = got[j][b].cpu().numpy()
            assert red.view(np.uint32) == have.view(np.uint32), (KEYS[j], b, k, red, have)


def test_devices_fan_out_and_drop_in(rows):
    pm.devices_fan_out(f"Spectral-{rows[0]}")


def test_cpu_mode_agrees(rows):
    pm.cpu_mode_agrees(f"Spectral-{rows[0]}")


def test_abi_on_the_device():
    lib = _native.load()
    x = torch.zeros(4, 8000, device="cuda")
    o = torch.zeros(3, 4, device="cuda")
    fr = torch.zeros(3, 4, 130, device="cuda")
    p = ctypes.c_void_p
    args = (p(x.data_ptr()), p(x.data_ptr()), 4, 8000, 8000, None)
    outs = tuple(p(o[k].data_ptr()) for k in range(3))
    for sr in (3999, 22050, 200000):
        assert lib.fsem_spectral_f32(*args, sr, p(fr.data_ptr()), 130, *outs, None) == _native.FSEM_ERATE
    assert lib.fsem_spectral_f32(*args, 8000, p(fr.data_ptr()), 129, *outs, None) == _native.FSEM_EINVAL  # F = 130
    assert lib.fsem_spectral_f32(*args[:2], 0, *args[3:], 8000, p(fr.data_ptr()), 130, *outs, None) == _native.FSEM_OK
    torch.cuda.synchronize()
    assert (o == 0).all() and (fr == 0).all()
    # length == 0: no frame kernel, every score NaN; a silent batch: every frame and score NaN
    assert lib.fsem_spectral_f32(args[0], args[1], 4, 0, 8000, None, 8000, p(fr.data_ptr()), 1, *outs, None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and (fr == 0).all()
    assert lib.fsem_spectral_f32(*args, 8000, p(fr.data_ptr()), 130, *outs, None) == _native.FSEM_OK
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and torch.isnan(fr).all()
