"""stoi_tob's third-octave envelopes and pesq_front's Bark bands and band-pass power against float64, element by
element (statements, norms, cases and yardsticks: tests/stage_cases.py; the statements themselves are held to
the pinned oracle by tests/test_stage_bands_cpu.py), through fsem_stoi_tob_f32 and fsem_pesq_front_f32.

Every bar is FACTOR = 4 times a float32 statement's own error against float64 on the same rows, evaluated on the
CPU; none comes from the engine's output.  Bars:
  tob    kept exact; every element of tob[:, :, :T] under the neighbour norm within 4 x the family's yardstick, and in
         the spectra family, whose cases' yardsticks differ 3000-fold (speech 2.6e-6, DC + 100 7e-3), within 4 x the
         case's own too; the level-gap family's quiet frames under the own-frame norm within 4 x the paired float32
         statement's at the 2^-6 step; exact zeros where a frame is zero; columns from T on untouched.
  front  power within 4 x the float32 statement's relative error; every Bark element of bands 1..48 under the
         neighbour norm within 4 x the family's yardstick, and band by band within 4 x the family's per-band yardstick
         (any float32 statement, pesq_front's own order of the pre-emphasis among them: the float32 recursions cost
         band 1 6e-2 and band 38 2e-6); band 0 absolutely against the statement (exact
         zeros); a seam's frames no worse than 2 x the interior's; ragged rows and batch positions bitwise.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from . import stage_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
FACTOR = sc.FACTOR


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fast_speech_enhancement_metrics_amd import _native
    return _native, _native.load(), torch.device("cuda:0")


def run_tob(eng, clean, deg):
    """(kept [B], tob [2B, 15, tmax + 3]) of 10 kHz rows [B, L]; tob starts out as SENTINEL."""
    _native, lib, dev = eng
    c = torch.from_numpy(np.array(clean)).to(dev)
    n = torch.from_numpy(np.array(deg)).to(dev)
    B, L = c.shape
    assert L % 4 == 0
    tmax = max((L - 256) // 128 + 1 - 2, 1) + 3
    kept = torch.full((B,), -1, dtype=torch.int32, device=dev)
    tob = torch.full((2 * B, 15, tmax), SENTINEL, device=dev)
    ws = _native.workspace(lib.fsem_stoi_workspace_bytes(B, L, 10000), dev)
    _native.check(lib.fsem_stoi_tob_f32(c.data_ptr(), n.data_ptr(), B, L, L, kept.data_ptr(), tob.data_ptr(), tmax,
                                        ws.data_ptr(), ws.numel(), _native.stream_handle(dev)), "tob")
    torch.cuda.synchronize()
    return kept.cpu().numpy(), tob.cpu().numpy()


def run_front(eng, ref, deg, lengths=None, plant_nan=False):
    """(bark [2B, 49, Fld], power [2B]) of 16 kHz rows [B, L].  ``lengths``: the ragged form; ``plant_nan``: NaN in
    both operands past each row's ceil4(length)."""
    _native, lib, dev = eng
    B, L = ref.shape
    ld = (L + 3) // 4 * 4
    ops = []
    for x in (ref, deg):
        t = torch.zeros(B, ld)
        t[:, :L] = torch.from_numpy(np.array(x))
        if plant_nan:
            for b in range(B):
                t[b, (int(lengths[b]) + 3) // 4 * 4:] = float("nan")
        ops.append(t.to(dev).contiguous())
    F = lib.fsem_pesq_frames(L)
    bark = torch.full((2 * B, 49, (F + 31) // 32 * 32), SENTINEL, device=dev)
    power = torch.full((2 * B,), SENTINEL, device=dev)
    lens = None if lengths is None else torch.tensor([int(v) for v in lengths], dtype=torch.int32, device=dev)
    ws = _native.workspace(lib.fsem_pesq_front_workspace_bytes(B, L), dev)
    _native.check(lib.fsem_pesq_front_f32(ops[0].data_ptr(), ops[1].data_ptr(), B, L, ld, _native.ptr(lens),
                                          bark.data_ptr(), power.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _native.stream_handle(dev)), "front")
    torch.cuda.synchronize()
    return bark.cpu().numpy(), power.cpu().numpy()


@pytest.fixture(scope="module")
def tob_got(eng):
    return {name: run_tob(eng, c["clean"], c["deg"]) for name, c in sc.tob_cases().items()}


@pytest.fixture(scope="module")
def front_got(eng):
    return {name: run_front(eng, c["ref"], c["deg"]) for name, c in sc.front_cases().items()}


# ------------------------------------------------------------------------------------------ stoi_tob
def _tob_errors(name, got):
    """Neighbour-norm errors per row of a case: list of [2, 15, T]."""
    exp = sc.tob_expected(name)
    _, tob = got
    B = len(exp["ref"])
    out = []
    for b, ref in enumerate(exp["ref"]):
        T = ref.shape[2]
        out.append(sc.neighbour_err(np.stack([tob[b][:, :T], tob[B + b][:, :T]]), ref, sc.PHI_TOB))
    return out


@pytest.mark.parametrize("name", list(sc.tob_cases()))
def test_tob_case(tob_got, name):
    case, exp = sc.tob_cases()[name], sc.tob_expected(name)
    kept, tob = tob_got[name]
    B = case["clean"].shape[0]
    assert kept.tolist() == exp["kept"]
    yard_f, yard_c = sc.tob_yardstick(case["family"]), max(exp["yard"].values())
    errs = _tob_errors(name, tob_got[name])
    for b, err in enumerate(errs):
        T = exp["ref"][b].shape[2]
        for s, sig in enumerate((b, B + b)):
            assert (tob[sig][:, max(T, 0):] == SENTINEL).all(), (b, s)   # columns from T on are untouched
            if T <= 0:
                continue
            j, t = np.unravel_index(err[s].argmax(), err[s].shape)
            print(f"{name} row {b} {'clean' if s == 0 else 'degraded'}: T {T}, largest error {err[s].max():.2e} (band "
                  f"{j}, frame {t}); yardstick: family {yard_f:.2e}, case {yard_c:.2e}; ratio "
                  f"{err[s].max() / yard_f:.2f}")
            assert np.isfinite(tob[sig][:, :T]).all()
            assert err[s].max() <= FACTOR * yard_f, (b, s, j, t)
            if case["family"] == "spectra":
                assert err[s].max() <= FACTOR * yard_c, (b, s, j, t)
    if "quiet" in case:  # level steps: the quiet side of each step under the own-frame norm
        bar = FACTOR * sc.own_frame_yardstick()
        for b, k in enumerate(sc.LEVEL_STEPS):
            T = exp["ref"][b].shape[2]
            err = sc.own_err(tob[B + b][:, :T], exp["ref"][b][1])[:, case["quiet"]]
            print(f"{name} step 2^-{k} at frame {case['t']}: quiet frames' own-frame error {err.max():.2e}; paired "
                  f"float32 statement at 2^-6 {sc.own_frame_yardstick():.2e}")
            assert err.max() <= bar, (k, np.unravel_index(err.argmax(), err.shape))
    if "zero_runs" in case:
        for b, (t0, cnt) in enumerate(case["zero_runs"]):
            z = tob[B + b][:, t0:t0 + cnt]
            assert (z == 0).all() and not np.signbit(z).any(), (t0, cnt)
            assert (tob[B + b][:, t0 - 1] > 0).all() and (tob[B + b][:, t0 + cnt] > 0).all()


def test_tob_batch_position(eng, tob_got):
    """A row's envelopes do not depend on the batch it is in: the spectra cases row by row, bitwise."""
    for name, case in sc.tob_cases().items():
        if case["family"] != "spectra":
            continue
        kept, tob = tob_got[name]
        B = case["clean"].shape[0]
        for b in range(B):
            k1, t1 = run_tob(eng, case["clean"][b:b + 1], case["deg"][b:b + 1])
            assert k1[0] == kept[b]
            np.testing.assert_array_equal(t1[0], tob[b])
            np.testing.assert_array_equal(t1[1], tob[B + b])


def _score():
    path = os.path.join(os.path.dirname(__file__), "..", "tools", "probes", "tob_compare.py")
    spec = importlib.util.spec_from_file_location("tob_compare", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.score


def test_tob_dc_attribution(tob_got):
    """Prints, for the DC + 100 and DC + 1000 rows, per band the engine's error beside the float32 statements',
    the statements' with one stage in float64, and the STOI that float64 segment math gives with one side's
    envelopes the engine's.  The assertion is the family bar of test_tob_case."""
    score = _score()
    fmt = lambda v: " ".join(f"{x:.0e}" for x in v)  # noqa: E731
    for name in ("spec_dc100", "spec_dc1000"):
        case, exp = sc.tob_cases()[name], sc.tob_expected(name)
        _, tob = tob_got[name]
        B = case["clean"].shape[0]
        errs = _tob_errors(name, tob_got[name])
        for b in range(B):
            ref = exp["ref"][b]
            T = ref.shape[2]
            print(f"{name} row {b} (T {T}), largest neighbour-norm error per band, clean then degraded")
            print("  engine              ", fmt(errs[b][0].max(1)), "|", fmt(errs[b][1].max(1)))
            for f in sc.FORMS:
                e = sc.neighbour_err(exp["f32"][f][b], ref, sc.PHI_TOB)
                print(f"  float32 {f:<12}", fmt(e[0].max(1)), "|", fmt(e[1].max(1)))
            for stage in ("ola", "fft", "bands"):
                got = sc.tob_rows(case["clean"][b], case["deg"][b], np.float32, "pair0", promote=stage)[1]
                e = sc.neighbour_err(got, ref, sc.PHI_TOB)
                print(f"  pair0, {stage:<5} float64", fmt(e[0].max(1)), "|", fmt(e[1].max(1)))
            ex, ey = tob[b][:, :T], tob[B + b][:, :T]
            print(f"  STOI of float64 envelopes {score(ref[0], ref[1]):+.6f}; engine clean, float64 degraded "
                  f"{score(ex, ref[1]):+.6f}; float64 clean, engine degraded {score(ref[0], ey):+.6f}; engine both "
                  f"{score(ex, ey):+.6f}")
            assert max(errs[b][0].max(), errs[b][1].max()) <= FACTOR * sc.tob_yardstick("spectra")


# ------------------------------------------------------------------------------------------ pesq_front
def _front_errors(name, got):
    """(per signal [48, F] neighbour-norm errors of bands 1..48, per signal band 0 absolute error, power errors)."""
    exp = sc.front_expected(name)
    bark, power = got
    errs, band0, perr = [], [], []
    for s, ref in enumerate(exp["bark"]):
        F = ref.shape[0]
        g = bark[s][:, :F].T           # [F, 49]
        assert np.isfinite(g).all()
        errs.append(sc.bark_err(g, ref))
        band0.append(float(np.abs(g[:, 0].astype(np.float64) - ref[:, 0]).max()))
        perr.append(abs(float(power[s]) - exp["power"][s]) / exp["power"][s])
    return errs, band0, perr


@pytest.mark.parametrize("name", list(sc.front_cases()))
def test_front_case(front_got, name):
    case, exp = sc.front_cases()[name], sc.front_expected(name)
    fam = case["family"]
    yard, yard_p = sc.front_yardstick(fam)
    band = sc.front_band_yardstick(fam)
    errs, band0, perr = _front_errors(name, front_got[name])
    for s, e in enumerate(errs):
        j, t = np.unravel_index(e.argmax(), e.shape)
        ratio = (e.max(1) / band)
        print(f"{name} signal {s}: F {e.shape[1]}, power error {perr[s]:.2e} (yardstick {yard_p:.2e}); Bark: largest "
              f"error {e.max():.2e} (band {j + 1}, frame {t}; yardstick {yard:.2e}, ratio {e.max() / yard:.2f}); "
              f"largest ratio to a band's yardstick {ratio.max():.2f} (band {ratio.argmax() + 1}); band 0 {band0[s]:.0e}")
    for s, e in enumerate(errs):
        assert perr[s] <= FACTOR * yard_p, s
        assert e.max() <= FACTOR * yard, s
        assert (e.max(1) <= FACTOR * band).all(), (s, np.nonzero(e.max(1) > FACTOR * band)[0] + 1)
        assert band0[s] <= FACTOR * exp["yard_band0"], s
    F = errs[0].shape[1]
    if F > sc.SEAM_FRAMES[0]:  # more than one segment: the frames at a seam against the others
        per_frame = np.max([e.max(0) for e in errs], 0)
        seam = np.zeros(F, bool)
        seam[[f for f in sc.SEAM_FRAMES if f < F]] = True
        if (~seam).any():
            print(f"{name}: largest error at a seam {per_frame[seam].max():.2e}, elsewhere "
                  f"{per_frame[~seam].max():.2e}")
            assert per_frame[seam].max() <= 2 * per_frame[~seam].max()


@pytest.mark.parametrize("group", range(len(sc.RAGGED)))
def test_front_ragged(eng, front_got, group):
    """Rows of different lengths in one batch with NaN past each row's ceil4(length): each row bitwise the row run
    alone at its own length, nothing of the NaNs in the output."""
    _native, lib, dev = eng
    lengths = sc.RAGGED[group]
    Lmax = max(lengths)
    ref = np.zeros((len(lengths), Lmax), np.float32)
    deg = np.zeros_like(ref)
    for b, L in enumerate(lengths):
        c = sc.front_cases()[f"len_{L}"]
        ref[b, :L], deg[b, :L] = c["ref"][0], c["deg"][0]
    bark, power = run_front(eng, ref, deg, lengths=lengths, plant_nan=True)
    B = len(lengths)
    for b, L in enumerate(lengths):
        b1, p1 = front_got[f"len_{L}"]
        F = sc.frames_of(L)
        for s, sig in enumerate((b, B + b)):
            assert np.isfinite(bark[sig][:, :F]).all() and np.isfinite(power[sig])
            np.testing.assert_array_equal(bark[sig][:, :F], b1[s][:, :F], err_msg=f"length {L} signal {s}")
            assert power[sig] == p1[s], (L, s)


def test_front_batch_position(eng, front_got):
    """The spectra rows one pair at a time: bitwise the batch's."""
    case = sc.front_cases()["spec"]
    bark, power = front_got["spec"]
    B, F = case["ref"].shape[0], sc.frames_of(sc.FRONT_SPEC_L)
    for b in range(B):
        b1, p1 = run_front(eng, case["ref"][b:b + 1], case["deg"][b:b + 1])
        for s, sig in enumerate((b, B + b)):
            np.testing.assert_array_equal(b1[s][:, :F], bark[sig][:, :F], err_msg=sc.FRONT_SPEC_ROWS[sig])
            assert p1[s] == power[sig]
