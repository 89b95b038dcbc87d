"""The pair metrics (``scores(clean, denoised, lengths=)``: LSD, SDR, BSSSDR, Composite, SpectralMeasures),
each described once, and what all of them promise, each promise stated once as a function of a
(metric, rate) id such as "LSD" or "Composite-8000".

A description names the metric's own cases module for everything numerical: its parity rows, its
float64 expectation and its checker with its tolerance constants are called here, not copied.  Two calls
that must give the same scores are compared bit for bit; a call is held to the float64 definition by
the metric's own checker (``close``).  tests/test_metric_contract_gpu.py and the metrics' own test files
call these bodies; a new pair metric adds one entry to PAIR_METRICS and one-line tests that name it."""
import copy
import ctypes
import functools
import pickle
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from fast_speech_enhancement_metrics_amd import BSSSDR, LSD, SDR, Composite, SpectralMeasures, _native

from . import bsssdr_cases as bc
from . import composite_cases as cc
from . import contract
from . import lsd_cases as lc
from . import sdr_cases as sc
from . import spectral_cases as sp
from .contract import bits, columns

NAN, INF = float("nan"), float("inf")
EINVAL, ERATE, EWORKSPACE = _native.FSEM_EINVAL, _native.FSEM_ERATE, _native.FSEM_EWORKSPACE


@dataclass(frozen=True)
class PairMetric:
    cls: type
    rates: tuple
    rows: Callable      # sr -> host (clean, noisy): the metric's parity rows
    expect: Callable    # (clean, noisy, sr, lengths=None) -> what `close` compares with (float64 definition)
    close: Callable     # (got, want, what): the metric's own checker at its own tolerance constants
    agree: Callable     # (gpu, cpu, want, what): the engine against CPU mode, at the metric's own constants
    poison: tuple       # (operand, row, column, value) of the non-finite rows
    fan_lengths: Callable  # (W, sr) -> the lengths of the fan-out, on the first len() rows
    layout_lengths: Callable = None  # W -> (L with L % 4 != 0, L4 < W): the two widths of `layouts`
    dtypes: bool = False             # layouts: float64 and int16 operands as well
    grid_rows: Callable = None       # -> host (clean, noisy) [4, 600]: the rows repeated past grid.y
    nonfinite_expected: bool = False  # non-finite rows: the whole batch against the definition as well
    frames: dict = None              # fan-out: a second form of the call (SpectralMeasures' frames)
    alone: tuple = None              # CPU mode's non-finite rows: (-> four host rows, the NaN's column)
    # the C entry on device pointers: (loader, prefix, arguments by name, outputs, row length, the size query's
    # further arguments, (override, code) table given the queried size)
    entry: tuple = None

    @property
    def keys(self):
        return self.cls.KEYS


def _composite_expect(c, n, sr, lengths=None):
    return c, n, sr, lengths, cc.expected_llr_wss(c, n, sr, lengths)


def _composite_agree(gpu, cpu, want, what):
    g, h = cc.to_np(gpu), cc.to_np(cpu)
    for name, k, atol in (("LLR", 4, cc.ATOL_LLR), ("WSS", 5, cc.ATOL_WSS), ("SegSNR", 6, sc.ATOL_SEG)):
        err = float(np.abs(h[k] - g[k]).max())
        print(f"{what} {name}: worst difference {err:.3e}")
        assert err <= atol, (name, h[k], g[k])


def _spectral_rows(sr):
    c, n = sp.parity_rows(sr)
    assert sp.frames_of(c.shape[1], sr) == sp.frames_of(c.shape[1] - 1, sr)  # the last sample is in no frame
    return c, n


def _spectral_expect(c, n, sr, lengths=None):
    return c, n, sr, lengths, sp.expected(c, n, sr, lengths)


def _spectral_agree(gpu, cpu, want, what):
    g, h = sp.to_np(gpu), sp.to_np(cpu)
    for k, name in enumerate(sp.KEYS):
        err = float(np.abs(h[k] - g[k]).max())
        print(f"{what} {name}: worst difference {err:.3e}")
        assert err <= sp.ATOL[name], (name, h[k], g[k])


def _bsssdr_rows(sr):
    (cs, ns), (cw, nw) = bc.speech_rows(4, 32000), bc.white_rows(4, 32000)  # 4 speech-like, 4 white
    return torch.cat([cs, cw]), torch.cat([ns, nw])


def _short_workspace_or_stride(size):
    return [(dict(ws_bytes=16), EWORKSPACE), (dict(ws_bytes=size - 1), EWORKSPACE), (dict(ld=999), EINVAL)]


_TAIL = (("n", 1, 12345, NAN), ("c", 2, -1, INF))    # (the last sample: in the tail of the last chunk or frame)
_TAIL_5000 = (("n", 1, 5000, NAN), ("c", 2, -1, INF))
_ONE_OUT = "ref deg batch length ld lengths o0 ws ws_bytes"

PAIR_METRICS = {
    "LSD": PairMetric(
        LSD, (16000,), rows=lambda sr: lc.speech_rows(4, 48000),
        expect=lambda c, n, sr, lengths=None: lc.expected(c, n, lengths), close=lc.assert_close,
        agree=lambda gpu, cpu, want, what: lc.assert_close(gpu, cpu.double().numpy(), what),
        poison=_TAIL, nonfinite_expected=True, fan_lengths=lambda W, sr: [48000, 1000, 30001, 479],
        layout_lengths=lambda W: (30001, 30000), dtypes=True, grid_rows=lambda: lc.speech_rows(4, 600, seed=23),
        alone=(lambda: lc.speech_rows(4, 8000), 4000),
        entry=(_native.load_lsd, "fsem_lsd", _ONE_OUT, 1, 1000, (), _short_workspace_or_stride)),
    "SDR": PairMetric(
        SDR, (16000,), rows=lambda sr: sc.speech_rows(4, 48000, 16000, snr_high=40),
        expect=lambda c, n, sr, lengths=None: sc.expected(c, n, sr, lengths=lengths), close=sc.assert_close,
        agree=lambda gpu, cpu, want, what: sc.assert_close(gpu, np.stack([v.double().numpy() for v in cpu]), what),
        poison=_TAIL, fan_lengths=lambda W, sr: [48000, 1000, 30001, 479],
        layout_lengths=lambda W: (30001, 30000), dtypes=True,
        grid_rows=lambda: sc.speech_rows(4, 600, 16000, seed=23), alone=(lambda: sc.speech_rows(4, 8000, 16000), 4000),
        entry=(_native.load, "fsem_sdr", "ref deg batch length ld lengths sr zm o0 o1 o2 ws ws_bytes", 3, 1000,
               (16000,),
               lambda size: [(dict(sr=3999), ERATE), (dict(ws_bytes=16), EWORKSPACE)])),
    "BSSSDR": PairMetric(
        BSSSDR, (16000,), rows=_bsssdr_rows,
        expect=lambda c, n, sr, lengths=None: bc.expected(c, n, lengths),
        close=lambda got, want, what: bc.assert_close(got, *want, what),
        agree=lambda gpu, cpu, want, what: bc.assert_close(gpu, cpu.double().numpy(), want[1], what),
        poison=_TAIL + (("n", 5, 0, -INF),), fan_lengths=lambda W, sr: [32000, 1000, 30001, 600],
        layout_lengths=lambda W: (30001, 30000), grid_rows=lambda: bc.white_rows(4, 600, seed=23),
        alone=(lambda: bc.white_rows(4, 4000), 2000),
        entry=(_native.load_bsssdr, "fsem_bsssdr", _ONE_OUT, 1, 1000, (), _short_workspace_or_stride)),
    "Composite": PairMetric(
        Composite, (8000, 16000), rows=cc.parity_rows, expect=_composite_expect,
        close=lambda got, w, what: cc.assert_scores(got, *w[:3], lengths=w[3], what=what, want=w[4]),
        agree=_composite_agree, poison=_TAIL_5000, fan_lengths=lambda W, sr: [W, 3000, W - 1, 479],
        layout_lengths=lambda W: (W - 3, W - 400), alone=(lambda: cc.parity_rows(16000), 4000),
        entry=(_native.load_composite, "fsem_composite",
               "ref deg batch length ld lengths sr o0 o1 o2 o3 o4 o5 o6 ws ws_bytes", 7, 8000, (16000,),
               lambda size: [(dict(sr=3999), ERATE), (dict(sr=22050), ERATE), (dict(sr=200000), ERATE),
                             (dict(ws_bytes=16), EWORKSPACE)])),
    "Spectral": PairMetric(
        SpectralMeasures, (8000, 16000), rows=_spectral_rows, expect=_spectral_expect,
        close=lambda got, w, what: sp.assert_scores(got, *w[:3], lengths=w[3], what=what, want=w[4]),
        agree=_spectral_agree, poison=_TAIL_5000,
        fan_lengths=lambda W, sr: [W, 3000, W - 1, 4 * sc.hop_win(sr)[0] - 1], frames=dict(return_frames=True)),
}


def ids(held=lambda d: True) -> list:
    """The ids ("LSD", "Composite-8000", ...) of the (metric, rate) pairs whose description ``held`` accepts."""
    return [name if len(d.rates) == 1 else f"{name}-{sr}"
            for name, d in PAIR_METRICS.items() if held(d) for sr in d.rates]


@functools.lru_cache(maxsize=None)
def case(key: str):
    """(description, rate, clean, noisy, expectation) of an id: host rows, built once and never written to."""
    name, _, rate = key.partition("-")
    d = PAIR_METRICS[name]
    sr = int(rate) if rate else d.rates[0]
    c, n = d.rows(sr)
    return d, sr, c, n, d.expect(c, n, sr)


@functools.lru_cache(maxsize=None)
def metric(key):
    """The id's metric on the engine, one per session."""
    d, sr = case(key)[:2]
    return d.cls(sr, use_gpu=True)


def same_bits(d, got, want, what):
    """contract.assert_bitwise with the metric's keys in the message (a further output is "frames")."""
    contract.assert_bitwise(got, want, what, names=d.keys + ("frames",))


def take(out, idx):
    """Rows ``idx`` of every output."""
    return [o[idx] for o in columns(out)]


# ------------------------------------------------------------------ on the engine
def layouts(key):
    """Scores do not depend on how the rows lie in memory, on their dtype or on the stream."""
    d, sr, c, n, _ = case(key)
    m = metric(key)
    B, W = c.shape
    L, L4 = d.layout_lengths(W)
    assert L % 4 and L4 < W
    cg, ng = c.cuda(), n.cuda()
    base = m.scores(cg[:, :L].contiguous(), ng[:, :L].contiguous())  # L % 4 != 0
    d.close(base, d.expect(c[:, :L], n[:, :L], sr), f"gpu {key} L={L}")
    same_bits(d, m.scores(cg[:, :L], ng[:, :L]), base, "strided view, L % 4 != 0")
    v = m.scores(cg[:, :L4], ng[:, :L4])  # ld = W > L, no copy
    d.close(v, d.expect(c[:, :L4], n[:, :L4], sr), "gpu strided view")
    same_bits(d, m.scores(cg[:, :L4].contiguous(), ng[:, :L4].contiguous()), v, "ld > L")
    # rows that do not start on 16-byte boundaries: the 4-byte loads give the same bits
    wide_c, wide_n = torch.zeros(B, W + 3, device="cuda"), torch.zeros(B, W + 3, device="cuda")
    wide_c[:, 1:L4 + 1], wide_n[:, 1:L4 + 1] = cg[:, :L4], ng[:, :L4]
    same_bits(d, m.scores(wide_c[:, 1:L4 + 1], wide_n[:, 1:L4 + 1]), v, "unaligned rows")
    if d.dtypes:
        same_bits(d, m.scores(cg[:, :L4].double(), ng[:, :L4].double()), v, "float64 input")
        ci, ni = (c[:, :L4] * 32768).round(), (n[:, :L4] * 32768).round()
        i16 = m.scores(ci.cuda().to(torch.int16), ni.cuda().to(torch.int16))
        d.close(i16, d.expect(ci, ni, sr), "gpu int16 input")
        same_bits(d, i16, m.scores(ci.cuda(), ni.cuda()), "int16 input")
    s = contract.on_side_stream(lambda: m.scores(cg[:, :L], ng[:, :L]))
    same_bits(d, s, base, "side stream")


def nonfinite_rows(key):
    """NaN in exactly the poisoned rows; the other rows are the clean batch's, bit for bit."""
    d, sr, c, n, _ = case(key)
    m = metric(key)
    c2, n2 = c.clone(), n.clone()
    for operand, row, column, value in d.poison:
        (c2 if operand == "c" else n2)[row, column] = value
    bad = sorted({p[1] for p in d.poison})
    good = [b for b in range(c.shape[0]) if b not in bad]
    base, got = m.scores(c.cuda(), n.cuda()), m.scores(c2.cuda(), n2.cuda())
    for g in columns(got):
        assert torch.isnan(g[bad]).all()
    same_bits(d, take(got, good), take(base, good), "finite rows beside non-finite ones")
    if d.nonfinite_expected:
        d.close(got, d.expect(c2, n2, sr), "gpu non-finite")


def past_grid_limit(key):
    """65537 rows of 600 samples (more than grid.y takes) against the four distinct rows."""
    d, sr = case(key)[:2]
    m = metric(key)
    NB = 65537
    c, n = d.grid_rows()
    cg, ng = c.cuda(), n.cuda()
    small = m.scores(cg, ng)
    reps = -(-NB // 4)
    big = m.scores(cg.repeat(reps, 1)[:NB].contiguous(), ng.repeat(reps, 1)[:NB].contiguous())
    src = np.arange(NB) % 4
    for g, w in zip(bits(columns(big)), bits(columns(small))):
        np.testing.assert_array_equal(g, w[src])
    d.close(small, d.expect(c, n, sr), "gpu 600-sample rows")


def assert_list_is(res, scores, keys):
    """The drop-in call's list: the keys in order, every value the float32 score."""
    host = [v.cpu().numpy() for v in columns(scores)]
    assert [tuple(r) for r in res] == [keys] * len(res) and len(res) == len(host[0])
    for b, r in enumerate(res):
        for k, key in enumerate(keys):
            np.testing.assert_array_equal(np.float32(r[key]), host[k][b])


def devices_fan_out(key):
    """devices=[0, 0] scores as one device does, without and with lengths; the drop-in call's list is the
    scores; copies and pickles of a fanned-out metric score alike."""
    d, sr, c, n, _ = case(key)
    m = metric(key)
    m2 = d.cls(sr, use_gpu=True, devices=[0, 0])
    lens = d.fan_lengths(c.shape[1], sr)
    c, n = c[:len(lens)], n[:len(lens)]
    cg, ng = c.cuda(), n.cuda()
    same_bits(d, m2.scores(cg, ng), m.scores(cg, ng), "devices=[0, 0]")
    one = m.scores(cg, ng, lengths=lens)
    same_bits(d, m2.scores(cg, ng, lengths=lens), one, "devices=[0, 0] with lengths")
    if d.frames:
        same_bits(d, m2.scores(cg, ng, lengths=lens, **d.frames), m.scores(cg, ng, lengths=lens, **d.frames),
                       f"devices=[0, 0] with {d.frames}")
    for call in (m, m2):
        assert_list_is(call(cg, ng, lengths=lens), one, d.keys)
    # lists of utterances
    assert_list_is(m([c[b, :k].cuda() for b, k in enumerate(lens)], [n[b, :k].cuda() for b, k in enumerate(lens)]),
                   one, d.keys)
    # copies and pickles drop what the metric keeps between calls (pinned buffers, the held list, the
    # fan-out's threads) and rebuild it on use
    for m3 in (copy.copy(m2), copy.deepcopy(m), pickle.loads(pickle.dumps(m2))):
        assert type(m3) is d.cls and m3.sample_rate == sr
        same_bits(d, m3.scores(cg, ng, lengths=lens), one, "a copied metric")
        assert_list_is(m3(cg, ng, lengths=lens), one, d.keys)


def cpu_mode_agrees(key):
    """CPU mode within the checker's bars of the definition, the engine within the metric's bars of CPU mode."""
    d, sr, c, n, want = case(key)
    cpu = d.cls(sr, use_gpu=False).scores(c, n)
    d.close(cpu, want, f"cpu {key}")
    d.agree(metric(key).scores(c.cuda(), n.cuda()), cpu, want, f"gpu vs cpu mode {key}")


def refuses_before_launch(key):
    """The C entry on device pointers refuses bad rates, strides and short workspaces, and writes no output."""
    loader, prefix, names, nout, L, query, table = PAIR_METRICS[key].entry
    lib = loader()
    x = torch.zeros(4, L, device="cuda")
    o = torch.zeros(nout, 4, device="cuda")
    size = getattr(lib, prefix + "_workspace_bytes")(4, L, *query)
    assert size > 0
    ws = torch.zeros(size, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p
    ok = dict(ref=p(x.data_ptr()), deg=p(x.data_ptr()), batch=4, length=L, ld=L, lengths=None, sr=16000, zm=0,
              ws=p(ws.data_ptr()), ws_bytes=size, **{f"o{k}": p(o[k].data_ptr()) for k in range(nout)})
    contract.refusals(contract.by_name(getattr(lib, prefix + "_f32"), names, None), ok, table(size))
    torch.cuda.synchronize()
    assert not o.any()  # (nothing ran)


# ------------------------------------------------------------------ without a GPU
def nonfinite_row_is_nan_alone(key):
    """CPU mode: NaN in the two poisoned rows, the other two bit for bit what they are in the clean batch."""
    d = PAIR_METRICS[key]
    rows, column = d.alone
    c, n = rows()
    n2, c2 = n.clone(), c.clone()
    n2[1, column] = NAN
    c2[3, 17] = INF
    m = d.cls(16000)
    base, got = m.scores(c, n), m.scores(c2, n2)
    for g in columns(got):
        assert torch.isnan(g[[1, 3]]).all()
    same_bits(d, take(got, [0, 2]), take(base, [0, 2]), "finite rows beside non-finite ones")
    if d.nonfinite_expected:
        d.close(got, d.expect(c2, n2, 16000), "cpu non-finite")


def one_output_validation(llib, name: str):
    """fsem_<name>_f32 (one output: LSD, BSSSDR) validates its arguments on the host; returns (accepted call's
    arguments, queried workspace size) for a library's further entries."""
    p, big, over = ctypes.c_void_p(16), 1 << 40, (1 << 29) + 4
    size = getattr(llib, f"fsem_{name}_workspace_bytes")(4, 160000)
    assert size > 0
    ok = dict(ref=p, deg=p, batch=4, length=160000, ld=160000, lengths=None, out=p, ws=p, ws_bytes=big)
    table = [(o, EINVAL) for o in (
        dict(ref=None, deg=None, out=None, ws=None, ws_bytes=0), dict(ref=None), dict(deg=None), dict(out=None),
        dict(batch=0), dict(length=0, ld=0), dict(ld=159999), dict(batch=1, length=over, ld=over, ws_bytes=1 << 62))]
    table += [(o, EWORKSPACE) for o in (dict(ws_bytes=16), dict(ws_bytes=size - 1), dict(ws=None))]
    names = "ref deg batch length ld lengths out ws ws_bytes"
    contract.refusals(contract.by_name(getattr(llib, f"fsem_{name}_f32"), names, None), ok, table)
    return ok, size
