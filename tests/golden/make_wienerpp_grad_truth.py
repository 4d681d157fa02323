"""Writes tests/golden/wienerpp_grad_truth.json: the 40-digit (mpmath) values of every output family of the pin problem of
tests/wienerpp_grad_truth_mp.py (N = 24, D = 3, M = 6), as decimal strings of 25 significant digits.

    python tests/golden/make_wienerpp_grad_truth.py      (a few seconds; needs mpmath)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import conftest  # noqa: E402,F401  (registers the product package, as under pytest)
import wienerpp_grad_truth_mp as WM  # noqa: E402

if __name__ == "__main__":
    out = {"digits": WM.DIGITS, "pin": WM.pin_values()}
    path = os.path.join(HERE, "wienerpp_grad_truth.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
