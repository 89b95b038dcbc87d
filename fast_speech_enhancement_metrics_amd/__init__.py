"""MI355X-native batched PESQ-wb, STOI/ESTOI, LSD and BSS-eval SDR (drop-in for kcoost/fast_speech_enhancement_metrics).

    from fast_speech_enhancement_metrics_amd import PESQ, STOI
    PESQ(sample_rate=16000, use_gpu=True)(clean, denoised)  -> [{"PESQ": ...}, ...]
    STOI(sample_rate=16000, use_gpu=True)(clean, denoised)  -> [{"STOI": ..., "ESTOI": ...}, ...]
    PESQ_STOI(16000, use_gpu=True)(clean, denoised)        -> [{"PESQ", "STOI", "ESTOI"}, ...]  (one pass)
    SDR(sample_rate=16000, use_gpu=True)(clean, denoised)   -> [{"SI-SDR", "SNR", "SegSNR"}, ...]  (extension)
    LSD(sample_rate=16000, use_gpu=True)(clean, denoised)   -> [{"LSD": ...}, ...]  (the reference's LSD)
    BSSSDR(sample_rate=16000, use_gpu=True)(clean, denoised) -> [{"SDR": ...}, ...]  (the reference's SDR)
    DNSMOS(sample_rate=16000, use_gpu=True)(None, denoised) -> [{"SIG", "BAK", "OVRL"}, ...]  (the reference's DNSMOS)
    Composite(16000, use_gpu=True)(clean, denoised)        -> [{"CSIG", "CBAK", "COVL", "PESQ", "LLR", "WSS", "SegSNR"}, ...]  (extension)
    SpectralMeasures(16000, use_gpu=True)(clean, denoised) -> [{"fwSegSNR", "CD", "IS"}, ...]  (extension)
    SRMR(sample_rate=16000, use_gpu=True)(None, denoised)   -> [{"SRMR": ...}, ...]  (extension, no reference signal)
    BSSEval(16000, use_gpu=True)(sources, estimates)       -> [{"SDR", "SIR", "SAR"}, ...]  (extension; [B, S, L] mixtures)
    PITSDR(16000, use_gpu=True)(sources, estimates)        -> [{"SI-SDR", "SNR"}, ...]  (extension; best assignment, .loss() is differentiable)

Ragged batches: pass lists of 1-D utterances, or padded [B, L] tensors with ``lengths=``.
"""
from .base import BaseMetric
from .PESQ import PESQ
from .STOI import STOI
from .joint import PESQ_STOI
from .SDR import SDR
from .Composite import Composite
from .Spectral import SpectralMeasures
from .LSD import LSD
from .BSSSDR import BSSSDR
from .BSSEval import BSSEval
from .PITSDR import PITSDR
from .DNSMOS import DNSMOS
from .SRMR import SRMR
from .alignment import time_align

__all__ = ["BaseMetric", "PESQ", "STOI", "PESQ_STOI", "SDR", "Composite", "SpectralMeasures", "LSD", "BSSSDR", "BSSEval",
           "PITSDR", "DNSMOS", "SRMR", "time_align"]
