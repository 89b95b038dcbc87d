"""Utterance-mode time alignment on the GPU (fsem_time_align_utt_f32, csrc/align.hip stages 5-9)
against the oracle (oracle/align_oracle.py steps 5-9; PARITY UNPINNED against P.862
implementations -- the reference has no time alignment, PESQ.py:19-22): segments, segment
delays, row delays equal to the oracle's and to the known per-utterance delays of
tests/align_cases.py (a delay change inside one utterance included), aligned rows bitwise the
oracle's segment shift, ragged and empty rows, PESQ(time_align="utterance") equal to the engine's
PESQ of the aligned rows, and a 512 x 10 s batch of the cases' kind."""
import time

import numpy as np
import pytest
import torch

from fast_speech_enhancement_metrics_amd.alignment import time_align, time_align_segments
from oracle import align_oracle as A
from tests import align_cases as AC
from tests import contract

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return contract.device()


def _check(res, want, B):
    al, dl, ns, st, sd = (t.cpu().numpy() for t in res)
    out, ds, segs = want
    np.testing.assert_array_equal(dl, ds)
    for b in range(B):
        s_o, d_o = segs[b]
        k = int(ns[b])
        np.testing.assert_array_equal(st[b, :k + 1], s_o)
        np.testing.assert_array_equal(sd[b, :k], d_o)
    np.testing.assert_array_equal(al, out)


def test_engine_matches_oracle(dev):
    c, d = AC.batch()
    want = A.align_utterances(c, d)
    res = time_align_segments(torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev))
    _check(res, want, c.shape[0])
    for (st, dl), case in zip(want[2], AC.CASES):
        assert list(dl) == case[3]


def test_engine_ragged_empty_and_bounded(dev):
    c, d = AC.batch(seed0=11)
    lens = [AC.L_UTT, 50000, 0, 700]
    want = A.align_utterances(c, d, lengths=lens)
    res = time_align_segments(torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev), lengths=lens)
    _check(res, want, c.shape[0])
    # a small max_delay bounds the crude lags (row and utterances) as in the oracle
    want = A.align_utterances(c, d, max_delay=256)
    res = time_align_segments(torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev), max_delay=256)
    _check(res, want, c.shape[0])


@pytest.mark.parametrize("mode", ["utterance", "p862"])
def test_engine_long_utterance_on_both_sides_of_its_lds_capacity(dev, mode):
    """One continuous utterance per row, 4200 and 4000 envelope frames long (seeds 21 and 22: the
    envelope cuts neither): ta_crude_utt stages search windows of up to 4096 frames in LDS and
    reads longer ones from global memory.  Both rows recover their known delay; delays, segments
    and aligned rows equal the package's CPU path."""
    L = 64 * 4200
    D = [700, -450]
    rows = [AC.continuous_pair(21 + b, L, [(0, L, D[b])]) for b in range(2)]
    c, d = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    lens = [L, 64 * 4000]
    g = [t.cpu().numpy() for t in time_align_segments(torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev),
                                                      lengths=lens, mode=mode)]
    h = [t.numpy() for t in time_align_segments(torch.from_numpy(c), torch.from_numpy(d), lengths=lens, mode=mode)]
    np.testing.assert_array_equal(h[1], D)
    np.testing.assert_array_equal(h[2], [1, 1])
    for b in range(2):
        np.testing.assert_array_equal(h[3][b, :2], [0, lens[b]])
    for i in (0, 1, 2):  # aligned rows, delays, n_seg
        np.testing.assert_array_equal(g[i], h[i])
    for b in range(2):
        np.testing.assert_array_equal(g[3][b, :2], h[3][b, :2])
        np.testing.assert_array_equal(g[4][b, :1], h[4][b, :1])


def test_pesq_utterance_mode(dev):
    from fast_speech_enhancement_metrics_amd import PESQ
    c, d = AC.batch()
    ct, dt = torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev)
    m = PESQ(16000, use_gpu=True, time_align="utterance")
    got = m.scores(ct, dt)
    al, ds = time_align(ct, dt, mode="utterance")
    want = PESQ(16000, use_gpu=True).scores(ct, al)
    torch.testing.assert_close(got, want, rtol=0, atol=0)
    np.testing.assert_array_equal(m.last_delays.cpu().numpy(), A.align_utterances(c, d)[1])


def test_engine_at_scale(dev):
    """512 rows x 10 s, each with 4 utterances at known delays (two per row pattern): every
    segment delay recovered; rows spot-checked against the oracle."""
    L = 160000
    utts = [(3000, 36000), (48000, 80000), (92000, 120000), (132000, 156000)]
    rng = np.random.default_rng(7)
    rows, dels = [], []
    for b in range(64):
        D = [int(x) for x in rng.integers(-1200, 1200, 4)]
        rows.append(AC.utt_pair(100 + b, L, utts, D))
        dels.append(D)
    c = np.stack([r[0] for r in rows] * 8)
    d = np.stack([r[1] for r in rows] * 8)
    ct, dt = torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev)
    time_align_segments(ct[:8], dt[:8])  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    al, dl, ns, st, sd = time_align_segments(ct, dt)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    print(f"utterance-mode alignment, 512 x 10 s: {ms:.2f} ms")
    ns, sd = ns.cpu().numpy(), sd.cpu().numpy()
    hit = 0
    for b in range(512):
        got = list(sd[b, :ns[b]])
        want = [x for i, x in enumerate(dels[b % 64]) if i == 0 or x != dels[b % 64][i - 1]]
        hit += got == want
    assert hit >= 0.95 * 512, hit
    for b in (0, 5, 63):
        out, ds, segs = A.align_utterances(c[b:b + 1], d[b:b + 1])
        np.testing.assert_array_equal(sd[b, :ns[b]], segs[0][1])
        np.testing.assert_array_equal(al[b].cpu().numpy(), out[0])


def test_engine_matches_cpu_path_on_random_plans(dev):
    """Random utterance plans (2-5 utterances, gaps 0.3-1 s, delays within +-1500 samples, a delay
    change inside one utterance in half the rows) at 10 s: the GPU's segments, delays and aligned
    rows against the package's float64 CPU path (the same algorithm) -- equal on >= 95 % of the
    rows (a VAD frame at its threshold can fall either side between float32 and float64
    envelopes; such rows must still agree on their row delay within one frame)."""
    from fast_speech_enhancement_metrics_amd.alignment import time_align_segments as tas
    L = 160000
    rng = np.random.default_rng(17)
    rows = []
    for b in range(24):
        nu = int(rng.integers(2, 6))
        t, utts = 2000, []
        for _ in range(nu):
            ln = int(rng.integers(16000, 36000))
            if t + ln > L - 2000:
                break
            utts.append((t, t + ln))
            t += ln + int(rng.integers(4800, 16000))
        D = [int(x) for x in rng.integers(-1500, 1500, len(utts))]
        split = None
        if b % 2 == 0:
            s0, e0 = utts[0]
            split = (0, (s0 + e0) // 2, D[0] + int(rng.choice([-1, 1])) * int(rng.integers(40, 300)))
        rows.append(AC.utt_pair(300 + b, L, utts, D, split))
    c = np.stack([r[0] for r in rows])
    d = np.stack([r[1] for r in rows])
    g = [t.cpu().numpy() for t in tas(torch.from_numpy(c).to(dev), torch.from_numpy(d).to(dev))]
    h = [t.numpy() for t in tas(torch.from_numpy(c), torch.from_numpy(d))]
    same = 0
    for b in range(len(rows)):
        k = int(g[2][b])
        eq = (k == int(h[2][b]) and np.array_equal(g[3][b, :k + 1], h[3][b, :k + 1])
              and np.array_equal(g[4][b, :k], h[4][b, :k]))
        if eq:
            np.testing.assert_array_equal(g[0][b], h[0][b])
        else:
            assert abs(int(g[1][b]) - int(h[1][b])) <= 64, (b, g[1][b], h[1][b])
        same += eq
    assert same >= 0.95 * len(rows), same
