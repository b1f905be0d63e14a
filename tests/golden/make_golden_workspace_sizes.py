#!/usr/bin/env python3
"""Record tests/golden/workspace_sizes.json: the workspace byte counts of the configurations in tests/workspace_cases.py.

Run from the repo root:   python tests/golden/make_golden_workspace_sizes.py [path/to/liblatentaug_hip.so]

The committed record was taken from the library built at commit 1e856d4, the last one BEFORE the metric entries' private layouts became
typed takes of LaCarver (la_common.h); its engine sizes are those recorded before the engines' own carvers were folded in, unchanged
since.  The test that reads it checks that neither fold moved a byte.  Re-record only when a layout changes on purpose, and from a
build that is trusted.  Needs no GPU: every call only computes a size.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402,F401  (its HIP runtime first, as _lib.load() does)
from latentaugment_amd import _lib  # noqa: E402
import workspace_cases  # noqa: E402

if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
sizes = workspace_cases.measure(_lib.load())
assert all(v > 0 for v in sizes.values()), [k for k, v in sizes.items() if v <= 0]
with open(os.path.join(HERE, 'workspace_sizes.json'), 'w') as f:
    json.dump(sizes, f, indent=0, sort_keys=True)
    f.write('\n')
print(len(sizes), 'sizes from', _lib.LOADED_PATH)
