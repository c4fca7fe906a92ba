#!/usr/bin/env python3
"""Record the launch sequence of ``functional`` into ``launch_trace.json`` (data only).

The trace of the PARENT of a change that rearranges the host code of ``functional`` is the oracle: check that commit out (with this
script and ``tests/test_gpu_launch_trace.py`` added: they need nothing but ``functional.call`` and ``_lib.PROTOTYPES``), build it and
run, from the repository root and on a machine WITH the GPU:

    python tests/golden/make_launch_trace.py

What is run and how a call is encoded: ``tests/test_gpu_launch_trace.py`` (the test records exactly this again)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else None
    import mau_amd
    from tests.test_gpu_launch_trace import CASES, GOLDEN, record_case
    cases = {name: record_case(mau_amd, case) for name, case in CASES.items()}
    with open(out or GOLDEN, "w") as f:             # one call per line: a changed call is one changed line
        f.write('{"cases": {\n')
        for k, (name, rows) in enumerate(cases.items()):
            f.write(f' {json.dumps(name)}: [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows) + "\n ]")
            f.write(",\n" if k + 1 < len(cases) else "\n")
        f.write("}}\n")
    print(f"{out or GOLDEN}: " + ", ".join(f"{name} {len(rows)}" for name, rows in cases.items()))
