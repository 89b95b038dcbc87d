"""Drop-in module path ``fast_se_metrics.LSD`` (reference fast_se_metrics/LSD.py)."""
from fast_speech_enhancement_metrics_amd.LSD import LSD  # noqa: F401

__all__ = ["LSD"]
