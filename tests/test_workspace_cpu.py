"""Workspace sizes are part of the ABI's observable behaviour: every fsem_*_workspace_bytes query
is pinned to tests/golden/workspace_bytes.json (recorded from the library of the commit named in
that file), and every entry that takes a workspace refuses one that is a byte short, before
anything launches.  No GPU is needed: the library answers these on the host.

The libraries beside libfsem.so (LSD, BSSSDR, Composite, DNSMOS) keep one golden file each,
tests/golden/<library>_workspace_bytes.json, on the same PAIRS.

    python -m tests.test_workspace_cpu        # re-record every golden file from the built libraries
"""
import ctypes
import json
import os
import subprocess

import pytest

from . import contract

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(REPO, "tests", "golden", "workspace_bytes.json")

PAIRS = [(1, 100), (1, 5376), (3, 40077), (7, 160000), (4096, 160000), (70000, 16000), (0, 160000)]
# (batch, length) queries of the entries without a rate
PLAIN = ["fsem_pesq_workspace_bytes", "fsem_pesq_front_workspace_bytes", "fsem_pesq_back_workspace_bytes",
         "fsem_pesq_distances_workspace_bytes", "fsem_pesq_stoi_workspace_bytes", "fsem_time_align_workspace_bytes",
         "fsem_time_align_utt_workspace_bytes", "fsem_time_align_p862_workspace_bytes",
         "fsem_pesq_bad_intervals_workspace_bytes"]
STOI_RATES = [8000, 10000, 16000, 48000]
# fsem_sdr_hop accepts 4000 ... 192000 Hz: the common rates and both ends at every pair, every
# accepted rate at (3, 40077) (run-length coded: the size is a step function of the rate), and
# the two nearest refused rates
SDR_RATES = [4000, 8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000]
SDR_REFUSED = [3999, 192001]
SDR_ALL = range(4000, 192001)
B, L, LD = 3, 40077, 40080  # the short-workspace case (the alignment entries take ld % 4 == 0)
OVER = (1 << 29) + 1  # a length past the engine's limit: every query answers 0


def library_golden(name: str) -> str:
    return os.path.join(REPO, "tests", "golden", f"{name}_workspace_bytes.json")


def record_library(name: str, lib) -> dict:
    """What tests/golden/<name>_workspace_bytes.json holds beside "pairs"."""
    if name == "composite":
        return {name: {str(sr): [lib.fsem_composite_workspace_bytes(b, l, sr) for b, l in PAIRS]
                       for sr in (8000, 16000, 7999, 22050)}}
    sizes = {name: [getattr(lib, f"fsem_{name}_workspace_bytes")(b, l) for b, l in PAIRS]}
    if name == "dnsmos":
        sizes.update(min=lib.fsem_dnsmos_min_workspace_bytes(), weights=lib.fsem_dnsmos_weights_bytes())
    return sizes


def _batch_and_length_limits(lib, golden, name):
    query = getattr(lib, f"fsem_{name}_workspace_bytes")
    assert all(golden[name][:-1]) and golden[name][-1] == 0  # (last pair: batch 0)
    assert query(4, 0) == 0 and query(1, OVER) == 0


def _composite_rates(lib, golden, name):
    assert all(golden[name]["16000"][:-1]) and all(golden[name]["8000"][:-1])  # (last pair: batch 0)
    assert not any(golden[name]["22050"]) and not any(golden[name]["7999"])


def _dnsmos_cap(lib, golden, name):
    """The recommended size stops growing at the cap on segments per pass."""
    from fast_speech_enhancement_metrics_amd import _native
    _batch_and_length_limits(lib, golden, name)
    assert lib.fsem_dnsmos_workspace_bytes(4096, 160000) == lib.fsem_dnsmos_workspace_bytes(70000, 1 << 20)
    assert golden["min"] < golden[name][4] <= _native.DNSMOS_MAX_PASS * golden["min"]


# library: what its test pinned beyond the recorded sizes
LIBRARIES = {"lsd": _batch_and_length_limits, "bsssdr": _batch_and_length_limits, "composite": _composite_rates,
             "dnsmos": _dnsmos_cap}


def record(lib) -> dict:
    sdr_runs = []
    for sr in SDR_ALL:
        n = lib.fsem_sdr_workspace_bytes(B, L, sr)
        if not sdr_runs or sdr_runs[-1][1] != n:
            sdr_runs.append([sr, n])
    return {
        "pairs": [list(p) for p in PAIRS],
        "plain": {name: [getattr(lib, name)(b, l) for b, l in PAIRS] for name in PLAIN},
        "stoi": {str(sr): [lib.fsem_stoi_workspace_bytes(b, l, sr) for b, l in PAIRS] for sr in STOI_RATES},
        "sdr": {str(sr): [lib.fsem_sdr_workspace_bytes(b, l, sr) for b, l in PAIRS] for sr in SDR_RATES + SDR_REFUSED},
        "sdr_every_rate": sdr_runs,  # [first rate, bytes] of each run of equal sizes at (B, L)
    }


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def up256(n: int) -> int:
    return (n + 255) // 256 * 256


def test_golden_covers_every_workspace_query(lib, golden):
    from fast_speech_enhancement_metrics_amd import _native
    queries = {n for n in _native.SIGNATURES if n.endswith("_workspace_bytes")}
    assert queries == set(PLAIN) | {"fsem_stoi_workspace_bytes", "fsem_sdr_workspace_bytes"}
    assert golden["pairs"] == [list(p) for p in PAIRS]
    assert [sr for sr in SDR_ALL if lib.fsem_sdr_hop(sr) == 0] == []
    assert all(lib.fsem_sdr_hop(sr) == 0 for sr in SDR_REFUSED)


def test_workspace_sizes_equal_the_recorded_ones(lib, golden):
    got = record(lib)
    assert got["plain"] == golden["plain"]
    assert got["stoi"] == golden["stoi"]
    assert any(v for v in golden["stoi"]["48000"]) and not any(golden["sdr"]["3999"])
    # SDR's last region was the one left unpadded: it may round up to a multiple of 256
    for sr, want in golden["sdr"].items():
        for (b, l), g, w in zip(PAIRS, got["sdr"][sr], want):
            assert g in (w, up256(w)), (sr, b, l, g, w)
    want_of = {}
    runs = golden["sdr_every_rate"]
    for (sr0, n), nxt in zip(runs, runs[1:] + [[SDR_ALL.stop, 0]]):
        for sr in range(sr0, nxt[0]):
            want_of[sr] = n
    assert sorted(want_of) == list(SDR_ALL)
    for sr in SDR_ALL:
        g = lib.fsem_sdr_workspace_bytes(B, L, sr)
        assert g in (want_of[sr], up256(want_of[sr])), (sr, g, want_of[sr])


@pytest.mark.parametrize("name", list(LIBRARIES))
def test_library_workspace_sizes_equal_the_recorded_ones(lib, name):
    from fast_speech_enhancement_metrics_amd import _native
    other = getattr(_native, f"load_{name}")()
    with open(library_golden(name)) as f:
        golden = json.load(f)
    assert golden["pairs"] == [list(p) for p in PAIRS]
    got = record_library(name, other)
    assert got == {k: golden[k] for k in got}
    LIBRARIES[name](other, golden, name)


def short_workspace_calls(lib):
    """(name, call(ws_bytes) -> rc, queried size) of every entry that takes a workspace, on (B, L)
    with non-null dummy pointers."""
    p, null = ctypes.c_void_p(16), None
    y_ld = ((5 * L + 7) // 8 + 3) // 4 * 4
    pesq = lib.fsem_pesq_workspace_bytes(B, L)
    front = lib.fsem_pesq_front_workspace_bytes(B, L)
    seg = (p, p, B, L, LD, null, 8000, p, p, p, p, p, LD, p)
    calls = [
        ("fsem_pesq_wb_f32", lambda n: lib.fsem_pesq_wb_f32(p, p, B, L, LD, null, p, p, n, null), pesq),
        ("fsem_pesq_wb_frames_f32", lambda n: lib.fsem_pesq_wb_frames_f32(p, p, B, L, LD, null, p, p, p, p, n, null),
         pesq),
        ("fsem_pesq_front_f32", lambda n: lib.fsem_pesq_front_f32(p, p, B, L, LD, null, p, p, p, n, null), front),
        ("fsem_pesq_front_y10_f32",
         lambda n: lib.fsem_pesq_front_y10_f32(p, p, B, L, LD, null, p, p, p, y_ld, null, 0, p, n, null), front),
        ("fsem_pesq_back_f32", lambda n: lib.fsem_pesq_back_f32(p, p, B, L, null, p, p, n, null),
         lib.fsem_pesq_back_workspace_bytes(B, L)),
        ("fsem_pesq_distances_f32", lambda n: lib.fsem_pesq_distances_f32(p, p, B, L, null, p, p, p, n, null),
         lib.fsem_pesq_distances_workspace_bytes(B, L)),
        ("fsem_stoi_tob_f32", lambda n: lib.fsem_stoi_tob_f32(p, p, B, L, LD, p, p, 1000, p, n, null),
         lib.fsem_stoi_workspace_bytes(B, L, 10000)),
        ("fsem_pesq_stoi_f32", lambda n: lib.fsem_pesq_stoi_f32(p, p, B, L, LD, null, p, p, p, p, n, null),
         lib.fsem_pesq_stoi_workspace_bytes(B, L)),
        ("fsem_time_align_f32", lambda n: lib.fsem_time_align_f32(p, p, B, L, LD, null, 8000, p, p, LD, p, n, null),
         lib.fsem_time_align_workspace_bytes(B, L)),
        ("fsem_time_align_utt_f32", lambda n: lib.fsem_time_align_utt_f32(*seg, n, null),
         lib.fsem_time_align_utt_workspace_bytes(B, L)),
        ("fsem_time_align_p862_f32", lambda n: lib.fsem_time_align_p862_f32(*seg, n, null),
         lib.fsem_time_align_p862_workspace_bytes(B, L)),
        ("fsem_pesq_bad_intervals_f32",
         lambda n: lib.fsem_pesq_bad_intervals_f32(p, p, p, B, L, LD, null, p, p, p, p, p, p, p, LD, p, n, null),
         lib.fsem_pesq_bad_intervals_workspace_bytes(B, L)),
        ("fsem_sdr_f32", lambda n: lib.fsem_sdr_f32(p, p, B, L, LD, null, 16000, 0, p, p, p, p, n, null),
         lib.fsem_sdr_workspace_bytes(B, L, 16000)),
    ]
    for sr in (8000, 10000, 16000):
        calls.append((f"fsem_stoi_f32@{sr}",
                      lambda n, sr=sr: lib.fsem_stoi_f32(p, p, B, L, LD, null, sr, p, p, p, n, null),
                      lib.fsem_stoi_workspace_bytes(B, L, sr)))
    return calls


def test_every_workspace_entry_is_exercised(lib):
    from fast_speech_enhancement_metrics_amd import _native
    takes_ws = {n for n, (_, args) in _native.SIGNATURES.items()
                if ctypes.c_size_t in args and not n.endswith("_workspace_bytes")}
    assert takes_ws == {name.split("@")[0] for name, _, _ in short_workspace_calls(lib)}


def test_a_workspace_one_byte_short_is_refused_before_any_launch(lib):
    # (no GPU here: a launch would come back as FSEM_ELAUNCH, not FSEM_EWORKSPACE)
    for name, call, size in short_workspace_calls(lib):
        assert size > 0, name
        assert call(size - 1) == -2, name


if __name__ == "__main__":
    from fast_speech_enhancement_metrics_amd import _build, _native
    _build.build()
    out = {"commit": subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True,
                                    check=True).stdout.strip()}
    out.update(record(_native.load()))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN)
    for name in LIBRARIES:
        with open(library_golden(name), "w") as f:
            sizes = record_library(name, getattr(_native, f"load_{name}")())
            json.dump({"pairs": [list(p) for p in PAIRS], **sizes}, f, separators=(",", ":"))
            f.write("\n")
        print("wrote", library_golden(name))
