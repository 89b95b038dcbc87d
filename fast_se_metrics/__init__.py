"""Drop-in import path of the reference package: ``from fast_se_metrics import PESQ, STOI``.

The package exports the hot-path metrics (PESQ-wb, STOI/ESTOI); LSD is provided under its module
path (``from fast_se_metrics.LSD import LSD``).  SDR, the 512-tap BSS-eval SDR, is provided under
its module path too (``from fast_se_metrics.SDR import SDR``), and so is DNSMOS
(``from fast_se_metrics.DNSMOS import DNSMOS``; its weights are a data file of this repository).
SpeechBERTScore of the reference is out of scope: its weights are a remote fetch.
"""
from fast_se_metrics.PESQ import PESQ  # noqa: F401  (module path first, then the class, as the reference)
from fast_se_metrics.STOI import STOI  # noqa: F401

__all__ = ["STOI", "PESQ"]
