"""Drop-in module path ``fast_se_metrics.SDR`` (reference fast_se_metrics/SDR.py): the 512-tap
BSS-eval SDR.  (The package's own ``SDR`` class, SI-SDR / SNR / SegSNR, is another metric.)"""
from fast_speech_enhancement_metrics_amd.BSSSDR import BSSSDR as SDR  # noqa: F401

__all__ = ["SDR"]
