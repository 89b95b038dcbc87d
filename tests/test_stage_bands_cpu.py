"""The references of tests/test_stage_bands_gpu.py alone (tests/stage_cases.py): the float64 statements against the
pinned oracle on the goldens, the cases' decisions, and the float32 yardsticks, which this file prints.

The oracle (oracle/stoi_oracle.py, oracle/pesq_oracle.py; pinned to the goldens by tests/test_oracle_golden.py)
rounds intermediates to float32 as the reference does: the overlap-added signal and the band powers for STOI, the
whole time-domain front end for PESQ.  The statements differ from it by that rounding and by nothing else, so the
bound of their agreement is that rounding, measured here between the oracle and the oracle's own steps written
out again with float64 carried through (``_oracle_tob_alt64`` / ``_oracle_bark_alt64``, numpy's transform and the
oracle's frame loop, not the statements' code), times 4.
"""
import numpy as np
import pytest
from scipy.signal import lfilter

from oracle import pesq_oracle as po
from oracle import stoi_oracle as so
from oracle import ta
from tests.conftest import load_golden

from . import stage_cases as sc


def _peak_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def _oracle_tob_alt64(x, y):
    """stoi_oracle.remove_silent_frames + third_octave_bands with no rounding to float32 -> (nk, [2, 15, T])."""
    w = so.window().astype(np.float64)
    n = (x.shape[0] - so.WIN) // so.HOP + 1
    idx = so.HOP * np.arange(n)[:, None] + np.arange(so.WIN)[None, :]
    e = so.frame_energies_db(x)
    keep = (e.max() - so.DYN_RANGE - e) < 0
    out = []
    for sig in (x, y):
        fr = (sig.astype(np.float64)[idx] * w)[keep]
        s = np.zeros((fr.shape[0] + 1) * so.HOP)
        for i in range(fr.shape[0]):
            s[i * so.HOP:i * so.HOP + so.WIN] += fr[i]
        win = np.zeros(so.N_FFT)
        win[128:384] = w
        nfr = 1 + (s.shape[0] - so.N_FFT) // so.HOP
        z = np.fft.rfft(s[so.HOP * np.arange(nfr)[:, None] + np.arange(so.N_FFT)[None, :]] * win, axis=1)
        p = z.real ** 2 + z.imag ** 2
        out.append(np.sqrt(np.stack([p[:, lo:hi].sum(1) for lo, hi in so.band_edges()], 0)))
    return int(keep.sum()), np.stack(out, 0)


def test_tob64_agrees_with_the_oracle():
    g = load_golden("stoi_10k")
    worst = [0.0, 0.0, 0.0]
    for b in range(g["clean_f"].shape[0]):
        x, y = g["clean_f"][b], g["noisy_f"][b]
        d = {}
        so.stoi_one(x, y, d)
        kept, tob = sc.tob64(x, y)
        nk, alt = _oracle_tob_alt64(x, y)
        assert kept == d["kept"] == nk == int(g["kept"][b])
        for s, key in enumerate(("tob_clean", "tob_noisy")):
            orc = d[key].astype(np.float64)
            worst[0] = max(worst[0], _peak_err(alt[s], orc))
            worst[1] = max(worst[1], _peak_err(tob[s], orc))
            worst[2] = max(worst[2], _peak_err(tob[s], alt[s]))
    print(f"stoi_10k: oracle's float32 rounding {worst[0]:.2e}; tob64 against the oracle {worst[1]:.2e}; tob64 "
          f"against the oracle's steps in float64 {worst[2]:.2e}")
    assert 0 < worst[0] < 1e-5
    assert worst[1] <= sc.FACTOR * worst[0]
    assert worst[2] < 1e-12


def _oracle_bark_alt64(speech):
    """pesq_oracle.get_bark_bands ([rows, L] float32, after equalize_ranges) with float64 carried through."""
    x = speech.astype(np.float64)
    filt = lfilter(po._BP_B.astype(np.float64), po._BP_A.astype(np.float64), x, axis=1)
    power = (filt ** 2).sum(1, keepdims=True) / (x.shape[1] + 5120) / 1.04684
    s = x * np.sqrt(1e7 / power)
    s[:, :15] *= po._TAPER
    s[:, -15:] *= po._TAPER[::-1]
    s = lfilter(po._PRE_B.astype(np.float64), po._PRE_A.astype(np.float64), s, axis=1)
    s = np.pad(s, ((0, 0), (0, s.shape[1] % 256)))
    nfr = 1 + (s.shape[1] - 512) // 256
    fr = s[:, 256 * np.arange(nfr)[:, None] + np.arange(512)[None, :]] * ta.hann_periodic(512).astype(np.float64)
    z = np.fft.rfft(fr, axis=2)
    p = z.real ** 2 + z.imag ** 2
    p[:, :, 0] = 0
    out = np.stack([p[:, :, po.BAND_EDGES[i]:po.BAND_EDGES[i + 1]].sum(2) for i in range(po.NBARK)], 2)
    return out * po.POW_DENS, power[:, 0]


def test_bark64_agrees_with_the_oracle():
    g = load_golden("pesq_3s")
    c, n = po.equalize_ranges(g["clean_f"], g["noisy_f"])
    speech = np.concatenate([c, n], 0)
    orc = po.get_bark_bands(speech)
    alt, alt_power = _oracle_bark_alt64(speech)
    L = speech.shape[1]
    worst = [0.0, 0.0, 0.0]
    for r in range(speech.shape[0]):
        power, bark = sc.bark64(speech[r])
        p = power / (L + 5120) / 1.04684
        scaled = bark * (1e7 / p)
        worst[0] = max(worst[0], _peak_err(alt[r], orc[r]))
        worst[1] = max(worst[1], _peak_err(scaled, orc[r]))
        worst[2] = max(worst[2], _peak_err(scaled, alt[r]), abs(p / alt_power[r] - 1))
    print(f"pesq_3s: oracle's float32 rounding {worst[0]:.2e}; bark64 against the oracle {worst[1]:.2e}; bark64 "
          f"against the oracle's steps in float64 {worst[2]:.2e}")
    assert 0 < worst[0] < 5e-3
    assert worst[1] <= sc.FACTOR * worst[0]
    # the oracle's Hann window is the float32 one (2^-24 of a sample, twice that in power, at most twice again
    # over a sum); the order-10 direct form against second-order sections in float64 is far below
    assert worst[2] < 2.0 ** -22


@pytest.mark.parametrize("name", list(sc.tob_cases()))
def test_tob_case_is_stable_under_its_selection(name):
    e = sc.tob_expected(name)
    print(name, "kept", e["kept"], f"margin {e['margin']:.3f} dB")
    assert e["margin"] >= sc.MARGIN_DB


def test_tob_cases_are_what_they_claim():
    cases = sc.tob_cases()
    for T_ in sc.EDGE_T:
        assert sc.tob_expected(f"edge_T{T_}")["kept"] == [T_ + 2]
    assert sc.tob_expected("edge_kept2")["kept"] == [2]
    keep = [sc.select64(r)[0] for r in cases["gaps"]["clean"]]
    assert not keep[0][0] and keep[0][1]
    assert not keep[1][-1] and keep[1][-2]
    assert keep[2][20:33].tolist() == [False, True] * 6 + [False]
    assert keep[3][24:31].tolist() == [False, False, False, True, False, False, False]
    for name, case in cases.items():
        if case["family"] == "levels":
            assert all(bool(sc.select64(r)[0].all()) for r in case["clean"]), name  # loud throughout
    # the zero runs: those frames of the statement are exact zeros, their neighbours are not
    ref = sc.tob_expected("level_zero_runs")["ref"]
    for r, (t0, cnt) in zip(ref, sc.ZERO_RUNS):
        assert (r[1][:, t0:t0 + cnt] == 0).all() and (r[1][:, t0 - 1] > 0).all() and (r[1][:, t0 + cnt] > 0).all()
        assert (r[0] > 0).all()


@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("parity", [0, 1])
def test_level_steps_move_the_peak_exponent_exactly(direction, parity):
    case = sc.tob_cases()[f"level_{direction}_{'even' if parity == 0 else 'odd'}"]
    t = case["t"]
    assert t % 2 == parity
    keep = np.ones((sc.LEVEL_L - 256) // 128 + 1, bool)
    for k, row in zip(sc.LEVEL_STEPS, case["deg"]):
        m, e = np.frexp(np.abs(sc.stft_frames(row, keep, np.float32)).max(1))
        assert (m > 0).all()
        loud, quiet = (t - 1, t) if direction == "down" else (t, t - 1)
        assert e[loud] - e[quiet] == k, (k, e[loud], e[quiet])
        # and the frames on the far side of the quiet one are quiet as well: the step is one step
        far = quiet + 1 if direction == "down" else quiet - 1
        assert abs(int(e[far]) - int(e[quiet])) <= 1


def test_tob_yardsticks():
    for fam in sc.TOB_FAMILIES:
        y = {f: max(sc.tob_expected(n)["yard"][f] for n, c in sc.tob_cases().items() if c["family"] == fam)
             for f in sc.FORMS}
        print(f"tob {fam}: float32 yardstick, neighbour norm: (a) {y['single']:.2e}  (b) even pairs {y['pair0']:.2e}"
              f"  (b) odd pairs {y['pair1']:.2e}  -> {sc.tob_yardstick(fam):.2e}")
        assert all(np.isfinite(v) and v > 0 for v in y.values())
        assert sc.tob_yardstick(fam) == max(y.values())
    for n, c in sc.tob_cases().items():
        if c["family"] == "spectra":
            print(f"  {n}: " + "  ".join(f"{f} {v:.2e}" for f, v in sc.tob_expected(n)["yard"].items()))
    y = sc.tob_expected("spec_speech")["yard"]
    for f in ("pair0", "pair1"):   # the emulation of the pair transform is itself sane
        assert y[f] <= sc.FACTOR * y["single"] and y["single"] <= sc.FACTOR * y[f]
    own = sc.own_frame_yardstick()
    print(f"tob levels: paired float32 statement, own-frame norm over the quiet frames of the 2^-6 steps: {own:.2e}")
    assert np.isfinite(own) and own > 0


def test_front_yardsticks():
    want = {5248: 20, 12544: 48, 12545: 48, 12671: 48, 12672: 49, 24832: 96, 25089: 97}
    for L, F in want.items():
        assert sc.frames_of(L) == F
    for fam in sc.FRONT_FAMILIES:
        for pre in sc.PRES:
            y = {f: max(sc.front_expected(n)["yard"][(pre, f)] for n, c in sc.front_cases().items()
                        if c["family"] == fam) for f in sc.FORMS}
            print(f"front {fam}, pre-emphasis order {pre}: float32 yardstick, neighbour norm: (a) {y['single']:.2e}  "
                  f"(b) even pairs {y['pair0']:.2e}  (b) odd pairs {y['pair1']:.2e}")
            assert all(np.isfinite(v) and v > 0 for v in y.values())
        yb, yp = sc.front_yardstick(fam)
        band = sc.front_band_yardstick(fam)
        print(f"front {fam}: Bark {yb:.2e}, power {yp:.2e}; per band 1..48: " + " ".join(f"{v:.0e}" for v in band))
        assert np.isfinite(yb) and yb > 0 and np.isfinite(yp) and yp > 0
        assert np.isfinite(band).all() and (band > 0).all()
    e = sc.front_expected("spec")
    for pre in sc.PRES:
        for f in ("pair0", "pair1"):
            a, b = e["yard"][(pre, "single")], e["yard"][(pre, f)]
            assert b <= sc.FACTOR * a and a <= sc.FACTOR * b
    # band 0 holds bin 0 alone, which is zeroed: the statements are exact zeros there
    assert all(x["yard_band0"] == 0 for x in map(sc.front_expected, sc.front_cases()))
