"""What a metric keeps between drop-in calls is process state: the per-thread pinned
score buffers (a threading.local), the last result list's fill handle (a PyCapsule) and the
fan-out's threads.  Copies and pickles of a metric drop it -- the reference's BaseMetric
(fast_se_metrics/base.py:6-43) is a plain object that can be copied -- and release() frees it."""
import copy
import pickle
import threading

import pytest
import torch

from fast_speech_enhancement_metrics_amd import BSSSDR, DNSMOS, LSD, PESQ, PESQ_STOI, SDR, STOI, Composite, _native

from . import bsssdr_cases as bc
from . import composite_cases as cc
from . import dnsmos_cases as dc
from . import lsd_cases as lc
from . import sdr_cases as sc


def randn_rows():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 16000, generator=g)
    return x, x + 0.1 * torch.randn(2, 16000, generator=g)


def keeps(*as_the_original, **attributes):
    """A metric's own check: the copy has these attribute values, and the original's of the named ones."""
    def own(m, original, rows):
        assert {k: getattr(m, k) for k in attributes} == attributes
        assert all(getattr(m, k) == getattr(original, k) for k in as_the_original)
    return own


def bsssdr_own(m, original, rows):
    assert m.filter_length == 512
    with pytest.raises(ValueError, match="pass sample_rate"):  # (an 8 kHz metric's scores() takes the rows' rate)
        m.scores(*rows)


# class: (how to make one in CPU mode, the call's operands, what a copy keeps beyond its class and rate)
STATE_CASES = {
    PESQ: (lambda: PESQ(16000, use_gpu=False), randn_rows, keeps()),
    STOI: (lambda: STOI(16000, use_gpu=False), randn_rows, keeps()),
    PESQ_STOI: (lambda: PESQ_STOI(16000, use_gpu=False), randn_rows, keeps()),
    LSD: (lambda: LSD(8000, use_gpu=False), lambda: lc.speech_rows(2, 12000, sr=8000), keeps(nfft=512)),
    SDR: (lambda: SDR(16000, use_gpu=False, zero_mean=True), lambda: sc.speech_rows(2, 16000, 16000),
          keeps(zero_mean=True)),
    BSSSDR: (lambda: BSSSDR(8000, use_gpu=False), lambda: bc.white_rows(2, 6000), bsssdr_own),
    Composite: (lambda: Composite(8000, use_gpu=False), lambda: cc.parity_rows(8000), keeps(lpc_order=10)),
    DNSMOS: (lambda: DNSMOS(16000, use_gpu=False), lambda: (None, dc.fixture("dnsmos_short").rows[:1]),
             keeps("weights_file")),
}


@pytest.mark.parametrize("cls", list(STATE_CASES), ids=lambda c: c.__name__)
def test_copy_and_pickle_drop_call_state(cls):
    make, rows, own = STATE_CASES[cls]
    rows, m = rows(), make()
    want = m(*rows)
    assert want == make()(*rows)
    # what a GPU call leaves behind (a native fill handle is a PyCapsule: neither copyable nor picklable)
    m.__dict__["_fsem_tls"] = threading.local()
    m.__dict__["_fsem_tls"].slots = {0: (torch.zeros(4),)}
    m.__dict__["_held_list"] = _native.score_list_alloc(2, ("PESQ",))[1]
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m)), copy.copy(m)):
        assert "_fsem_tls" not in c.__dict__ and "_held_list" not in c.__dict__
        assert c._fanout is None and c.sample_rate == m.sample_rate and type(c) is cls
        own(c, m, rows)
        assert c(*rows) == want  # the copy scores as the original


def test_release_drops_held_list_and_slots():
    m = PESQ_STOI(16000, use_gpu=False)
    m.release()  # nothing held yet: a no-op
    m.__dict__["_fsem_tls"] = threading.local()
    m.__dict__["_fsem_tls"].slots = {0: (torch.zeros(4),)}
    m.__dict__["_held_list"] = object()
    m.release()
    assert "_held_list" not in m.__dict__ and m.__dict__["_fsem_tls"].slots == {}
