#!/usr/bin/env python3
"""Golden vectors at 448 x 448 and 512 x 512 inputs by RUNNING THE REFERENCE (build container only):

    python tests/golden/gen_golden_hires.py [case ...]       # writes tests/golden/<case>.npz for tests/_hires_params.py

Same recipe, spies and tie-free checks as gen_golden.py (imported, not edited); only the case table differs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402  (sets up the reference import path and the timm stand-in)

from tests._hires_params import HIRES_CASES  # noqa: E402

if __name__ == "__main__":
    only = sys.argv[1:]
    for name, case in HIRES_CASES.items():
        if only and name not in only:
            continue
        gen_golden.run_case(name, case)
