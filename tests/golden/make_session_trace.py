#!/usr/bin/env python3
"""Record the launch sequence of the captured sessions and the test-split drivers into ``session_trace.json``, and the CSV files the
drivers write into ``session_trace_reports/`` (data only).

The trace of the PARENT of a change that rearranges the host code of the sessions or the drivers is the oracle: check that commit out
(with this script, ``tests/test_gpu_session_trace.py`` and ``tests/_helpers.py`` added: they need nothing but the sessions, the drivers,
``functional.call`` and ``_lib.PROTOTYPES``), build it and run, from the repository root and on a machine WITH the GPU:

    python tests/golden/make_session_trace.py

What is run and how a call is encoded: ``tests/test_gpu_session_trace.py`` (the test records exactly this again)."""
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    import mau_amd
    from tests.test_gpu_session_trace import CASES, GOLDEN, GOLDEN_REPORTS, REPORTS
    cases = {}
    for name, record in CASES.items():
        with tempfile.TemporaryDirectory() as work:
            cases[name] = record(mau_amd, work)
            if name == "eval_drivers":
                os.makedirs(GOLDEN_REPORTS, exist_ok=True)
                for report in REPORTS:
                    shutil.copyfile(os.path.join(work, "reports", report), os.path.join(GOLDEN_REPORTS, report))
    with open(GOLDEN, "w") as f:                    # one call per line: a changed call is one changed line
        f.write('{"cases": {\n')
        for k, (name, rows) in enumerate(cases.items()):
            f.write(f' {json.dumps(name)}: [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows) + "\n ]")
            f.write(",\n" if k + 1 < len(cases) else "\n")
        f.write("}}\n")
    print(f"{GOLDEN}: " + ", ".join(f"{name} {len(rows)}" for name, rows in cases.items()))
