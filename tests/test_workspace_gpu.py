"""No entry writes outside the workspace it asked for.  The caching allocator rounds every
allocation up, so a region laid out past the queried size would go unnoticed; here each workspace
is the first `nbytes` of a larger buffer whose 4096-byte tail is a guard pattern, the body starts
as 0xFF bytes (NaN floats, -1 ints: nothing may rely on what the allocator left there), and the
scores must equal the unguarded call's bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 3, 40077  # several PESQ segments (12288 samples) and alignment chunks (5120), L % 4 != 0
RAGGED = (40077, 20000, 6000)
GUARD = 4096


@pytest.fixture(scope="module")
def pair():
    from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs
    clean, noisy, _ = speech_like_pairs(B, L, 16000, seed=11, snr_low=0, snr_high=20)
    noisy = torch.roll(noisy, 240, dims=1)  # a delay for the alignment modes to find
    return clean.cuda(), noisy.cuda()


def _pesq(mode):
    def run(clean, noisy, lengths):
        from fast_speech_enhancement_metrics_amd import PESQ
        m = PESQ(16000, use_gpu=True, time_align=mode)
        mos = m.scores(clean, noisy, lengths)
        return (mos,) if not mode else (mos, m.last_delays)
    return run


def _stoi(sr):
    def run(clean, noisy, lengths):
        from fast_speech_enhancement_metrics_amd import STOI
        return STOI(sr, use_gpu=True).scores(clean, noisy, sr, lengths=lengths)
    return run


def _joint(clean, noisy, lengths):
    from fast_speech_enhancement_metrics_amd.joint import PESQ_STOI
    return PESQ_STOI(16000, use_gpu=True).scores(clean, noisy, lengths)


def _sdr(clean, noisy, lengths):
    from fast_speech_enhancement_metrics_amd.SDR import SDR
    return SDR(16000, use_gpu=True).scores(clean, noisy, lengths)


def _stages(clean, noisy, lengths):  # fsem_pesq_front_f32, then fsem_pesq_distances_f32
    from fast_speech_enhancement_metrics_amd import PESQ
    return PESQ(16000, use_gpu=True).frame_disturbances(clean, noisy, lengths)


CASES = {"pesq": _pesq(False), "pesq_row": _pesq("row"), "pesq_utterance": _pesq("utterance"),
         "pesq_p862": _pesq("p862"),  # also the bad-interval and pooling entries
         "stoi_16000": _stoi(16000), "stoi_10000": _stoi(10000), "stoi_8000": _stoi(8000),
         "pesq_stoi": _joint, "sdr": _sdr, "stages": _stages}


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("case", list(CASES))
def test_guarded_workspace_stays_intact_and_scores_are_bitwise_equal(case, ragged, pair, monkeypatch):
    from fast_speech_enhancement_metrics_amd import _native
    clean, noisy = pair
    lengths = torch.tensor(RAGGED, dtype=torch.int32) if ragged else None
    want = [t.clone() for t in CASES[case](clean, noisy, lengths)]
    torch.cuda.synchronize()

    handed = []

    def guarded(nbytes, device):
        n = max(int(nbytes), 1)
        buf = torch.empty(n + GUARD, dtype=torch.uint8, device=device)
        buf[:n] = 0xFF
        buf[n:] = 0xA5
        handed.append((buf, n))
        return buf[:n]

    monkeypatch.setattr(_native, "workspace", guarded)
    got = [t.clone() for t in CASES[case](clean, noisy, lengths)]
    torch.cuda.synchronize()
    assert handed, "the case took no workspace"
    for buf, n in handed:
        assert bool((buf[n:] == 0xA5).all()), f"{case}: a write past a workspace of {n} bytes"
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        # bit patterns, so that NaN scores (rows too short for a metric) compare equal to themselves
        assert torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), (case, g, w)
