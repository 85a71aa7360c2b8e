"""Writes tests/golden/preprocess_zoom.safetensors: `scipy.ndimage.zoom` along the middle axis of small fp64 arrays, for every
order, line length and factor tests/test_preprocess_cpu.py uses, so that a host without scipy still pins the restatement
(tests/preprocess_ref.py) and `preprocess.axis_taps`.  Needs scipy (the fixture was written with 1.15.3); run from the repository root:
    python tools/gen_preprocess_golden.py
"""
import os
import sys

import numpy as np
import torch
from safetensors.torch import save_file
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_preprocess_cpu import FACTORS, LENGTHS, ORDERS, zoom_input  # noqa: E402  (the cases are the test's)


def main():
    tensors = {}
    for n in LENGTHS:
        x = zoom_input(n)
        for f in FACTORS:
            if int(round(n * f)) < 1:
                continue
            for order in ORDERS:
                tensors[f"o{order}_n{n}_f{f}"] = torch.from_numpy(np.ascontiguousarray(ndimage.zoom(x, [1, f, 1], order=order)))
    path = os.path.join(ROOT, "tests", "golden", "preprocess_zoom.safetensors")
    import scipy
    save_file(tensors, path, metadata={"scipy": scipy.__version__, "call": "scipy.ndimage.zoom(x, [1, f, 1], order=order)"})
    print(path, os.path.getsize(path), "bytes,", len(tensors), "arrays")


if __name__ == "__main__":
    main()
