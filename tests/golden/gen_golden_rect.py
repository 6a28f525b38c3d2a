#!/usr/bin/env python3
"""Golden vectors at a rectangular input by RUNNING THE REFERENCE (build container only):

    python tests/golden/gen_golden_rect.py [case ...]       # writes tests/golden/<case>.npz for tests/_rect_params.GOLDEN_RECT

Same recipe, spies and tie-free checks as gen_golden.py (imported, not edited); the case table is tests/_rect_params.py's, and the
generator's int-only helpers (make_params, make_images, case_config) are replaced by that module's pair forms.  The timm stand-in's
PatchEmbed takes img_size=(H, W) as it is."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402  (sets up the reference import path and the timm stand-in)

from tests import _rect_params  # noqa: E402

if __name__ == "__main__":
    only = sys.argv[1:] or _rect_params.GOLDEN_RECT
    with _rect_params.patched(gen_golden):
        for name in only:
            gen_golden.run_case(name, _rect_params.RECT_CASES[name])
