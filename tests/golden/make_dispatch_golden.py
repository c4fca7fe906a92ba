#!/usr/bin/env python3
"""Record the dispatch decisions of a built library into ``dispatch_decisions.json`` (data only).

The decisions of the PARENT of a change to the launch rules are the oracle: build that commit somewhere, point ``MAU_LIB`` at its
``libmau_hip.so`` and run, from the repository root and on a host WITHOUT a GPU (the library then assumes 256 CUs / 8 XCDs):

    MAU_LIB=/path/to/parent/libmau_hip.so python tests/golden/make_dispatch_golden.py

What is swept and how it is encoded: ``tests/test_dispatch_decisions_host.py`` (the test recomputes exactly this)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    import mau_amd  # noqa: F401
    from mau_amd import _lib
    from tests.test_dispatch_decisions_host import GOLDEN, record
    doc = record(_lib)
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{GOLDEN}: recorded from {_lib.LIB_PATH}: {doc['count']}")
