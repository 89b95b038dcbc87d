"""The pair metrics' shared operand preparation (base.pair_rows, base.engine_rows) on the GPU: the
scores of SDR, Composite, LSD, BSSSDR, PESQ, STOI and the joint PESQ_STOI do not depend on how the
operands lie in memory, and rows of no samples score as each metric documents.

The engine headers promise scores independent of alignment and row capacity, so the reference is
the call on contiguous operands and the comparison is bitwise.  The layouts take every branch of
the padding rule: an odd element offset (bases not 16-byte aligned), different row strides for the
two operands, and a row stride that is no multiple of 4.  Every length but 260 is no multiple of 4
and is padded whatever the layout; at 260 (and Composite's 5248, and the 8196 of PESQ, STOI and the
joint call) the views themselves reach the engine unless the rule (or its 16-byte form) copies them.
PESQ, STOI and the joint call are scored at lengths that give every row a finite score (PESQ needs
20 frames, STOI a 30-frame segment at 10 kHz), so their comparison is one of numbers, not of NaNs."""
import pytest
import torch

from fast_speech_enhancement_metrics_amd import BSSSDR, DNSMOS, LSD, PESQ, PESQ_STOI, SDR, STOI, Composite, _cpu

from . import lsd_cases as lc

pytestmark = pytest.mark.gpu

B = 3
LENGTHS = (1, 5, 258, 260, 8193)
# Composite scores only rows PESQ has at least 20 frames for: its shortest length and the next one
SHORTEST = next(L for L in range(1, 1 << 14) if _cpu.pesq_frames(L) >= 20)
METRICS = {"SDR": (SDR, LENGTHS), "Composite": (Composite, (SHORTEST, SHORTEST + 1)), "LSD": (LSD, LENGTHS),
           "BSSSDR": (BSSSDR, LENGTHS)}
FINITE = (8193, 8196)  # every row of rows() has 20 PESQ frames and 8 STOI segments at both
METRICS.update({"PESQ": (PESQ, FINITE), "STOI": (STOI, FINITE), "PESQ_STOI": (PESQ_STOI, FINITE)})
# (a STOI(16000)'s scores() must be told its rows' rate)
RATE = {"STOI": (16000,)}


def rows(L: int):
    g = torch.Generator().manual_seed(1000 + L)
    clean = torch.randn(B, L, generator=g) * 0.1
    return clean.cuda(), (clean + 0.03 * torch.randn(B, L, generator=g)).cuda()


def in_buffer(x: torch.Tensor, width: int, offset: int) -> torch.Tensor:
    """x's values as the view buf[:, offset:offset + L] of a fresh [B, width] buffer."""
    buf = torch.full((x.shape[0], width), 7.0, device=x.device)  # (finite filler: never part of a score)
    view = buf[:, offset:offset + x.shape[1]]
    view.copy_(x)
    assert view.stride(0) == width and torch.equal(view, x)
    return view


def layouts(c: torch.Tensor, n: torch.Tensor):
    L = c.shape[1]
    w = L + 2 if (L + 2) % 4 else L + 3  # no multiple of 4, and holds L samples behind an offset of 1
    yield "odd element offset", in_buffer(c, L + 1, 1), in_buffer(n, L + 1, 1)
    yield "different row strides", in_buffer(c, L + 4, 0), in_buffer(n, L + 8, 0)
    yield "row stride no multiple of 4", in_buffer(c, w, 0), in_buffer(n, w, 0)
    yield "all three", in_buffer(c, w, 1), in_buffer(n, w + 2, 1)


def stacked(s) -> torch.Tensor:
    return torch.stack(list(s)) if isinstance(s, tuple) else s


def assert_same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), what
    assert torch.equal(got[~nan], want[~nan]), (what, (got - want).abs().max().item())


@pytest.mark.parametrize("name", list(METRICS))
def test_scores_do_not_depend_on_the_operands_layout(name):
    cls, lengths = METRICS[name]
    metric = cls(16000, use_gpu=True)
    rate = RATE.get(name, ())
    for L in lengths:
        c, n = rows(L)
        assert c.is_contiguous() and n.is_contiguous()
        want = stacked(metric.scores(c, n, *rate))
        assert want.shape[-1] == B
        if lengths is FINITE:
            assert want.isfinite().all(), (name, L, want)
        for what, cv, nv in layouts(c, n):
            assert_same(stacked(metric.scores(cv, nv, *rate)), want, f"{name} L={L}: {what}")
        assert_same(stacked(metric.scores(c, n, *rate)), want, f"{name} L={L}: repeated")


def test_rows_of_no_samples():
    c = torch.zeros(B, 0, device="cuda")
    zeros = torch.zeros(B, dtype=torch.int32)
    for got in (SDR(16000, use_gpu=True).scores(c, c), SDR(16000, use_gpu=True).scores(c, c, lengths=zeros),
                Composite(16000, use_gpu=True).scores(c, c, lengths=zeros)):
        got = stacked(got)  # (no launch: NaN in every score)
        assert got.is_cuda and got.shape[1] == B and got.isnan().all()
    with pytest.raises(RuntimeError, match="but size is 20"):  # (the whole-batch form, as PESQ's)
        Composite(16000, use_gpu=True).scores(c, c)
    # LSD and BSSSDR launch on four zero samples of length 0
    lsd = LSD(16000, use_gpu=True)
    lc.assert_close(lsd.scores(c, c), [lc.LN1E8] * B, "LSD, no samples")
    lc.assert_close(lsd.scores(c, c, lengths=zeros), [lc.LN1E8] * B, "LSD, no samples, lengths")
    bss = BSSSDR(16000, use_gpu=True)
    for got in (bss.scores(c, c), bss.scores(c, c, lengths=zeros)):
        assert got.is_cuda and got.shape == (B,) and got.isnan().all()
    got = DNSMOS(16000, use_gpu=True).scores(c)
    assert got.is_cuda and got.shape == (B, 3) and got.isnan().all()
    for metric in (lsd, bss):  # (and the drop-in call's list)
        res = metric(c, c)
        assert len(res) == B and all(set(r) == set(metric.KEYS) for r in res)
