"""What the metrics' tests share: the bitwise comparison, the library and device fixtures' bodies, the
side-stream idiom and the refusal tables of the C entries.  It imports neither torch nor the package
until a helper is used; the pair metrics' descriptions and shared test bodies are tests/pair_metrics.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_BIT_VIEWS = {np.dtype(np.float32): np.uint32, np.dtype(np.int32): np.int32, np.dtype(np.float64): np.uint64}


# ------------------------------------------------------------------ helpers
def columns(out) -> tuple:
    """A metric's output as a tuple of tensors (a one-score metric returns the tensor itself)."""
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def bits(t):
    """The bit patterns of a tensor (float32 as uint32, int32 as int32, float64 as uint64), or the
    list of them for a tuple of tensors: NaNs compare by their payload, zeros by their sign."""
    if isinstance(t, (tuple, list)):
        return [bits(v) for v in t]
    a = t.detach().cpu().contiguous().numpy()
    return a.view(_BIT_VIEWS[a.dtype])


def assert_bitwise(got, want, what="", names=None):
    g, w = columns(got), columns(want)
    assert len(g) == len(w), (what, len(g), len(w))
    for k, (a, b) in enumerate(zip(g, w)):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{what} {names[k] if names else k}")


def load_lib():
    """The ``lib`` fixture's body: libfsem.so, built from this tree if need be."""
    from fast_speech_enhancement_metrics_amd import _build, _native
    _build.build()
    return _native.load()


def device():
    """The ``dev`` fixture's body."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def on_side_stream(fn):
    """fn() on a fresh stream that waits for the current one; synchronised before it returns."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = fn()
    side.synchronize()
    return out


def by_name(cfunc, names: str, *tail):
    """A C entry as a function of named arguments, in the order of ``names``; ``tail`` follows them."""
    order = names.split()
    return lambda **a: cfunc(*(a[k] for k in order), *tail)


def refusals(fn, ok: dict, cases) -> None:
    """Every (override, code) of ``cases``: fn(**ok) with the override's arguments replaced returns code."""
    for over, code in cases:
        assert fn(**{**ok, **over}) == code, over


def each(code, *overrides):
    """[(override, code), ...]: one row of a refusal table per override."""
    return [(o, code) for o in overrides]


def nulled(code, names: str):
    """Each named pointer argument as NULL in turn."""
    return [({k: None}, code) for k in names.split()]


def entries_are_declared_exported_and_bound(lib, prefix: str, entries, others=()):
    """The names of libfsem.so that start with ``prefix`` are the same in include/fsem.h, in the library's exports
    and in _native.SIGNATURES: ``entries`` (what a metric added) and ``others`` (None: not pinned).  Each added
    entry is bound with its declared types, takes no size_t and is no workspace query: such entries join the
    library without a version bump."""
    from fast_speech_enhancement_metrics_amd import _build, _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fsem.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = {n for n in re.findall(r" T (fsem_[a-z0-9_]+)", out) if n.startswith(prefix)}
    declared = set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, header))
    bound = {n for n in _native.SIGNATURES if n.startswith(prefix)}
    assert exported == declared == bound and set(entries) <= bound
    if others is not None:
        assert bound == set(entries) | set(others)
    for name in entries:
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.restype is restype and fn.argtypes == argtypes
        assert ctypes.c_size_t not in argtypes and not name.endswith("_workspace_bytes")
        declared_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).strip()
        assert "size_t" not in declared_args
        assert (0 if declared_args in ("", "void") else declared_args.count(",") + 1) == len(argtypes)
    assert lib.fsem_version() == 11
