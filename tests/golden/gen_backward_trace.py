#!/usr/bin/env python3
"""Records the backward executor's launch trace (tests/_backward_trace.py) into tests/golden/backward_trace.json:

    python tests/golden/gen_backward_trace.py --commit $(git rev-parse HEAD)

Run it on the MI355X with the library built from the commit whose launch sequence is to be pinned; tests/test_backward_trace_gpu.py
compares later trees against the record.  Every case runs twice: the traces must agree, and the gradient hash is stored only when both
runs give the same one (a case that does not reproduce keeps its trace and gets "hash": null; it is printed).

The workspace is filled with 0xFF bytes before every recorded backward, and every trainable slice of the flat gradient buffer must come
out finite.  A case that fails this reads workspace it never wrote: it is recorded with a zero-filled workspace instead and named in the
header's "zero_workspace", which has to match _backward_trace.ZERO_WS (at most two cases, none of MUST_HASH) -- otherwise the file is
still written, for inspection, and the generator exits with an error.  A block-range case must give the bits of its single-call case.

Format: "records" is the table of distinct (label, flops, bytes); a case's "launches" are indices into it, in launch order."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import _backward_trace as bt  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under test was built from")
    ap.add_argument("--tr-train", default=os.path.join(ROOT, "tokenreduction_amd", "csrc", "tr_train.hip"),
                    help="the tr_train.hip the library under test was built from (hashed into the header)")
    a = ap.parse_args()
    with open(a.tr_train, "rb") as f:
        header = dict(commit=a.commit, tr_train_hip_sha256=hashlib.sha256(f.read()).hexdigest(), **bt.device_header())
    table, cases, lost, zero_ws, errors = {}, {}, [], [], []
    for name in bt.CASES:
        try:
            l1, h1, model = bt.run(name)
        except (RuntimeError, NotImplementedError, ValueError) as e:          # the case cannot take a training step: reported, the rest is recorded
            errors.append(f"{name}: {type(e).__name__}: {e}")
            print(errors[-1], flush=True)
            continue
        bad = bt.nonfinite_trainable(model)
        if bad:          # the backward read workspace it never wrote
            print(f"{name}: NOT FINITE under the 0xFF workspace: {bad[:6]}{' ...' if len(bad) > 6 else ''}; recorded with a zero-filled one", flush=True)
            zero_ws.append(name)
            l1, h1, _ = bt.run(name, poison=False)
        l2, h2, _ = bt.run(name, poison=not bad)
        if l1 != l2:
            errors.append(f"{name}: two runs enqueue different launches")
        if h1 != h2:
            lost.append(name)
        cases[name] = {"hash": h1 if h1 == h2 else None, "launches": [table.setdefault(rec, len(table)) for rec in l1]}
        print(f"{name}: {len(l1)} launches, hash {'ok' if h1 == h2 else 'NOT REPRODUCIBLE'}", flush=True)
    for name in bt.CASES:
        one = bt.single_call(name)
        if one and name in cases and one in cases and cases[name]["hash"] != cases[one]["hash"]:          # (two nulls: nothing to compare)
            errors.append(f"{name}: not the bits of {one}")
    header["zero_workspace"] = sorted(zero_ws)
    out = os.path.join(HERE, "backward_trace.json")
    with open(out, "w") as f:          # one case per line
        f.write('{"header": ' + json.dumps(header) + ',\n"records": ' + json.dumps([list(r) for r in table], separators=(",", ":")) + ',\n"cases": {\n')
        f.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in cases.items()))
        f.write("\n}}\n")
    print(f"backward_trace.json: {len(cases)} cases, {len(table)} distinct launches, {os.path.getsize(out)} bytes; without a hash: {lost}; "
          f"zero-filled workspace: {zero_ws}")
    assert not errors, errors
    assert len(lost) <= 2 and not set(lost) & set(bt.MUST_HASH), f"hashes that do not reproduce: {lost}"
    assert len(zero_ws) <= 2 and not set(zero_ws) & set(bt.MUST_HASH), f"cases that read unwritten workspace: {zero_ws}"
    assert sorted(zero_ws) == sorted(bt.ZERO_WS), f"_backward_trace.ZERO_WS = {bt.ZERO_WS}, found {zero_ws}"
