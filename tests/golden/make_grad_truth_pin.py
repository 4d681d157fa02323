"""Writes tests/golden/grad_truth_pin.npz: tests/grad_truth.py's outputs on the hand-written problem of
tests/grad_truth_pin.py.  Run it with the module whose bits are to be kept, never to make a failing pin pass."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from grad_truth_pin import grad_truth_pin  # noqa: E402

if __name__ == "__main__":
    pin = grad_truth_pin()
    np.savez_compressed(os.path.join(HERE, "grad_truth_pin.npz"), **pin)
    print(len(pin), "arrays")
