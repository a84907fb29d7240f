#!/usr/bin/env python3
"""Golden vector for the graded-matrix test of the resampling core -> tests/golden/resample_graded.npz.

``T0 = B D`` of tests/resample_cases.py (B Gaussian 64 x 33, D a shuffled 2^(-2j): singular values spanning 5e-20) and its
singular values by ``mpmath.svd_r`` at 60 digits, rounded to float64.  Stored because mpmath need not be installed where the
tests run; tests/test_resample_cases_host.py recomputes them where it is.

    python tools/gen_golden_resample.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import resample_cases as rc  # noqa: E402

T0 = rc.graded_matrix()[2]
sv = rc.graded_reference()
np.savez_compressed(rc.GOLDEN, T0=T0, sv=sv)
print(rc.GOLDEN, os.path.getsize(rc.GOLDEN), "bytes; sigma_1", sv[0], "sigma_r", sv[-1])
