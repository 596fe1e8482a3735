"""Helper of test_fm_kernels_gpu.py::test_fm_deterministic_matches_reference:
in a fresh process started with WH_DETERMINISTIC=1 (the mode is read once per
process), the deep-batch checks of tests/_fm_cases.py at vstride 16 and 64 on
valued data, with two backward calls on the same inputs compared bit for bit.
Prints the largest |err| / bound per quantity, then OK."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _fm_cases as fc  # noqa: E402
from wormhole_amd import _native  # noqa: E402

assert os.environ.get("WH_DETERMINISTIC") == "1", "run with WH_DETERMINISTIC=1"
dev = torch.device("cuda", 0)
hip = _native.hip()
localized = {}
for vstride in (16, 64):
    fc.run_depth_case(hip, dev, vstride, True, localized, deterministic=True, tag="det ")
torch.cuda.synchronize()
for name in sorted(fc.RATIOS):
    print("  RATIO %-12s %.3f" % (name, fc.RATIOS[name]))
print("OK")
