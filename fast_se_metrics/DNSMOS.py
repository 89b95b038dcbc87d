"""Drop-in module path ``fast_se_metrics.DNSMOS`` (reference fast_se_metrics/DNSMOS.py)."""
from fast_speech_enhancement_metrics_amd.DNSMOS import DNSMOS  # noqa: F401

__all__ = ["DNSMOS"]
