#!/usr/bin/env python3
"""Records what every registered factory constructs (tests/_construction.py) into tests/golden/model_construction.json:

    python tests/golden/gen_model_construction.py

Run it on the commit whose constructors are to be pinned; tests/test_model_construction.py compares later trees against the record."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _construction as con  # noqa: E402

if __name__ == "__main__":
    snaps = {key: con.snapshot(name, args) for key, name, args in con.cases()}
    mismatch = {which: con.mismatch_message(which) for which in con.MISMATCH_CASES}
    out = os.path.join(HERE, "model_construction.json")
    with open(out, "w") as f:          # one construction per line
        f.write('{"mismatch": ' + json.dumps(mismatch) + ',\n"entries": {\n')
        f.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in snaps.items()))
        f.write("\n}}\n")
    print(f"model_construction.json: {len(snaps)} constructions, {os.path.getsize(out)} bytes")
