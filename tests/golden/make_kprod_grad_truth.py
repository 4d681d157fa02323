"""Writes tests/golden/kprod_grad_truth.json: the 40-digit (mpmath) values tests/kprod_grad_truth.py is pinned to -- kind 20 and
its derivative over the nu and x grid of tests/kprod_grad_truth_mp.py, and every output family of the pin problem there (N = 24,
D = 3, M = 6) -- as decimal strings of 25 significant digits.

    python tests/golden/make_kprod_grad_truth.py      (about a minute; needs mpmath)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import kprod_grad_truth_mp as KM  # noqa: E402

if __name__ == "__main__":
    out = {"digits": KM.DIGITS, "bessel": KM.bessel_table(), "pin": KM.pin_values()}
    path = os.path.join(HERE, "kprod_grad_truth.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
