"""Every library of _build.LIBRARIES, without a GPU: it exports exactly the fsem_* symbols its header
declares, its binding table (_native.LIBRARY_SIGNATURES) lists the same, no other library or table
holds one of them, its header and sources are build dependencies, and it carries the tree's build id
and target."""
import os
import re
import subprocess

import pytest

from fast_speech_enhancement_metrics_amd import _build, _native

from . import contract

# the entry set of each library after the core, pinned name by name
ENTRIES = {
    "composite": {"fsem_composite_chunk", "fsem_composite_workspace_bytes", "fsem_composite_f32"},
    "lsd": {"fsem_lsd_frames", "fsem_lsd_chunk", "fsem_lsd_workspace_bytes", "fsem_lsd_f32"},
    "bsssdr": {"fsem_bsssdr_filter_length", "fsem_bsssdr_chunk", "fsem_bsssdr_norm_chunk",
               "fsem_bsssdr_workspace_bytes", "fsem_bsssdr_f32", "fsem_bsssdr_load_diag_f32"},
    "dnsmos": {"fsem_dnsmos_segments", "fsem_dnsmos_weights_bytes", "fsem_dnsmos_pack_weights_f32",
               "fsem_dnsmos_min_workspace_bytes", "fsem_dnsmos_workspace_bytes", "fsem_dnsmos_f32",
               "fsem_dnsmos_features_f32", "fsem_dnsmos_raw_f32"},
}


@pytest.fixture(scope="module")
def lib():
    return contract.load_lib()


def declared(entry) -> set:
    src = re.sub(r"/\*.*?\*/", "", open(_build.header_abi(entry)).read(), flags=re.S)
    return set(re.findall(r"\b(fsem_[a-z0-9_]+)\s*\(", src))


def exported(entry) -> set:
    out = subprocess.run(["nm", "-D", "--defined-only", _build.library_path(entry)], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r" T (fsem_[a-z0-9_]+)", out))


def test_the_table_is_the_five_libraries_in_build_order():
    assert [entry.name for entry in _build.LIBRARIES] == ["core", "composite", "lsd", "bsssdr", "dnsmos"]
    assert [entry.name for entry in _build.LIBRARIES] == list(_native.LIBRARY_SIGNATURES)
    assert [entry.name for entry in _build.LIBRARIES if entry.links_core] == ["composite"]
    assert [_build.library_path(entry) for entry in _build.LIBRARIES] == [
        _build.LIB, _build.COMPOSITE_LIB, _build.LSD_LIB, _build.BSSSDR_LIB, _build.DNSMOS_LIB] == [
        _native._DEFAULT_LIB, _native.COMPOSITE_LIB_PATH, _native.LSD_LIB_PATH, _native.BSSSDR_LIB_PATH,
        _native.DNSMOS_LIB_PATH]
    assert [_build.header_abi(entry) for entry in _build.LIBRARIES] == [
        _build.HEADER_ABI, _build.COMPOSITE_HEADER_ABI, _build.LSD_HEADER_ABI, _build.BSSSDR_HEADER_ABI,
        _build.DNSMOS_HEADER_ABI]
    assert [_native.LIBRARY_SIGNATURES[n] for n in ("core", "composite", "lsd", "bsssdr", "dnsmos")] == [
        _native.SIGNATURES, _native.COMPOSITE_SIGNATURES, _native.LSD_SIGNATURES, _native.BSSSDR_SIGNATURES,
        _native.DNSMOS_SIGNATURES]


@pytest.mark.parametrize("entry", _build.LIBRARIES, ids=lambda entry: entry.name)
def test_library_exports_what_its_header_declares(lib, entry):
    decl = declared(entry)
    assert decl, "no declarations parsed"
    if entry.name != "core":
        assert decl == ENTRIES[entry.name]
    assert exported(entry) == decl == set(_native.LIBRARY_SIGNATURES[entry.name])
    for other in _build.LIBRARIES:
        if other is not entry:
            assert not exported(other) & decl and not set(_native.LIBRARY_SIGNATURES[other.name]) & decl, other.name
    names = {os.path.basename(d) for d in _build.deps()}
    assert os.path.basename(_build.header_abi(entry)) in names and entry.sources and set(entry.sources) <= names
    path = _build.library_path(entry)
    assert _build.library_build_id(path) == _build.source_hash() == _native.build_id()
    assert _build.library_build_arch(path) == _build.ARCH
    assert not _build._stale()
    assert lib.fsem_version() == 11  # (libfsem.so is as it was: each later metric is a library of its own)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_engine_loader_binds_the_table_and_keeps_the_handle(lib, name):
    eng = _native.load_engine(name)
    assert eng is _native.load_engine(name) is getattr(_native, "load_" + name)() and eng is not lib
    for fname, (res, args) in _native.LIBRARY_SIGNATURES[name].items():
        fn = getattr(eng, fname)
        assert fn.restype is res and fn.argtypes == args


def test_engine_loader_refuses_what_the_tree_did_not_build(lib, monkeypatch, tmp_path):
    """A missing library, one of other sources and one for another target each raise ImportError in
    the loader's words, for every engine; nothing is rebuilt."""
    calls = []
    monkeypatch.setattr(_build, "build", lambda *a, **k: calls.append(1))
    monkeypatch.setattr(_native, "_engines", {})
    for entry in _build.LIBRARIES[1:]:
        what = f"fsem {entry.label} engine"
        with monkeypatch.context() as m:
            m.setattr(_build, "ARCH", "gfx942")
            with pytest.raises(ImportError, match=f"{what} .* was built for gfx950, this process targets gfx942"):
                _native.load_engine(entry.name)
        with monkeypatch.context() as m:
            flags = dict(_build.SOURCE_FLAGS, **{"pesq.hip": []})
            m.setattr(_build, "SOURCE_FLAGS", flags)
            with pytest.raises(ImportError, match=f"{what} .* is stale"):
                _native.load_engine(entry.name)
        with monkeypatch.context() as m:
            m.setattr(_build, "LIBDIR", str(tmp_path))
            with pytest.raises(ImportError, match=f"{what} not built: .* is missing"):
                _native.load_engine(entry.name)
    assert not calls and not _native._engines
    with pytest.raises(KeyError):
        _native.load_engine("srmr")
    with pytest.raises(ValueError):
        _native.load_engine("core")
