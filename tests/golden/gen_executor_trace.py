#!/usr/bin/env python3
"""Records the forward executor's launch trace (tests/_executor_trace.py) into tests/golden/executor_trace.json:

    python tests/golden/gen_executor_trace.py --commit $(git rev-parse HEAD)

Run it on the MI355X with the library built from the commit whose launch sequence is to be pinned; tests/test_executor_trace_gpu.py
compares later trees against the record.  Every case runs twice: the traces must agree, and the output hash is stored only when both
runs give the same one (a case that does not reproduce keeps its trace and gets "hash": null; it is printed).

Format: "records" is the table of distinct (label, flops, bytes); a case's "launches" are indices into it, in launch order."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import _executor_trace as et  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under test was built from")
    a = ap.parse_args()
    with open(os.path.join(ROOT, "tokenreduction_amd", "csrc", "tr_vit.hip"), "rb") as f:
        header = dict(commit=a.commit, tr_vit_hip_sha256=hashlib.sha256(f.read()).hexdigest(), **et.device_header())
    table, cases, lost = {}, {}, []
    for name in et.CASES:
        (l1, h1), (l2, h2) = et.run_case(name), et.run_case(name)
        assert l1 == l2, f"{name}: two runs enqueue different launches"
        if h1 != h2:
            lost.append(name)
        cases[name] = {"hash": h1 if h1 == h2 else None, "launches": [table.setdefault(rec, len(table)) for rec in l1]}
        print(f"{name}: {len(l1)} launches, hash {'ok' if h1 == h2 else 'NOT REPRODUCIBLE'}", flush=True)
    assert len(lost) <= 2 and not set(lost) & set(et.MUST_HASH), f"hashes that do not reproduce: {lost}"
    out = os.path.join(HERE, "executor_trace.json")
    with open(out, "w") as f:          # one case per line
        f.write('{"header": ' + json.dumps(header) + ',\n"records": ' + json.dumps([list(r) for r in table], separators=(",", ":")) + ',\n"cases": {\n')
        f.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in cases.items()))
        f.write("\n}}\n")
    print(f"executor_trace.json: {len(cases)} cases, {len(table)} distinct launches, {os.path.getsize(out)} bytes; without a hash: {lost}")
