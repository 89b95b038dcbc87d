"""Writes tests/golden/dnsmos_grad_basis.json: how far the gradient of the rounding emulation
(tests/dnsmos_grad_cases.py: the float64 graph carrying the engine's forward roundings) lies from the float64
gradient, on the rows of tests/golden/dnsmos_16k.npz and the three keys.  From the package alone, on the CPU.

    python -m tests.golden.make_dnsmos_grad_golden

    basis        the largest deviation of the gradient with respect to the samples
    basis_image  the same for the gradient with respect to the log-power image alone

The deviation is tests/dnsmos_grad_cases.deviation: the largest absolute deviation over the largest absolute
float64 element, per row and key.  The file holds these two results only.
"""
import json

import torch

from .. import dnsmos_cases as dc
from .. import dnsmos_grad_cases as gc


def measure(rows=None, keys=(0, 1, 2), verbose=True):
    """(basis, basis_image) over ``rows`` (indices into dnsmos_16k, all by default) and ``keys``."""
    fx = dc.fixture("dnsmos_16k")
    worst, worst_image = 0.0, 0.0
    for b in range(fx.rows.shape[0]) if rows is None else rows:
        _, want, want_i = gc.gradients(fx.rows[b], keys=keys, images=True)
        _, got, got_i = gc.gradients(fx.rows[b], network=gc.emulated_network, keys=keys, images=True)
        for j, k in enumerate(keys):
            d, di = gc.deviation(got[j], want[j]), gc.deviation(got_i[j], want_i[j])
            if verbose:
                print(f"row {b} {dc_key(k)}: samples {d:.3e} (max |g| {abs(want[j]).max():.3e}), image {di:.3e}")
            worst, worst_image = max(worst, d), max(worst_image, di)
    return worst, worst_image


def dc_key(k: int) -> str:
    return ("SIG", "BAK", "OVRL")[k]


if __name__ == "__main__":
    torch.manual_seed(0)
    basis, basis_image = measure()
    with open(gc.BASIS_FILE, "w") as f:
        json.dump({"basis": basis, "basis_image": basis_image}, f)
        f.write("\n")
    print("wrote", gc.BASIS_FILE, basis, basis_image)
