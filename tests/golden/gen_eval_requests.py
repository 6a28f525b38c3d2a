#!/usr/bin/env python3
"""Records how every public eval entry refuses a request (tests/_eval_requests.py) into tests/golden/eval_requests.json:

    python tests/golden/gen_eval_requests.py

Run it on the commit whose refusals are to be pinned; tests/test_eval_requests.py compares later trees against the record."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _eval_requests as req  # noqa: E402

if __name__ == "__main__":
    cells = req.matrix()
    out = os.path.join(HERE, "eval_requests.json")
    with open(out, "w") as f:          # one state per block, one call per line
        f.write('{"model": ' + json.dumps(req.MODEL) + ',\n"states": {\n')
        f.write(",\n".join(json.dumps(state) + ": {\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in row.items()) + "\n}"
                           for state, row in cells.items()))
        f.write("\n}}\n")
    print(f"eval_requests.json: {sum(len(r) for r in cells.values())} cells, {os.path.getsize(out)} bytes")
