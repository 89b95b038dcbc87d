"""The pair metrics' layouts and fan-out on the HIP engine (tests/pair_metrics.py), one case per (metric,
rate).  SpectralMeasures keeps a layouts test of its own (frames output, one length, the `ldf` step through
the C entry); BSSSDR's and SpectralMeasures' fan-out tests are in their own files."""
import pytest

from . import pair_metrics as pm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", pm.ids(lambda d: d.layout_lengths))
def test_layouts(key):
    pm.layouts(key)


@pytest.mark.parametrize("key", ["LSD", "SDR", "Composite-8000", "Composite-16000"])
def test_devices_fan_out(key):
    pm.devices_fan_out(key)
