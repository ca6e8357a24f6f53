#!/usr/bin/env python3
"""Record the workspace sizes the built library states, at the shapes of tests/workspace_cases.py, into workspace_bytes.json.

    python tests/golden/gen_workspace_bytes.py          # every case answers without a device

The file pins the ABI: a workspace a caller sized with an older build must stay large enough, and the offsets inside it are
part of the same contract.  It is regenerated only by a change that means to move a size, never to make a test pass.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from qrec_amd import capi  # noqa: E402
from workspace_cases import CPU_CASES, stated_bytes  # noqa: E402

path = os.path.join(HERE, "workspace_bytes.json")
doc = json.load(open(path)) if os.path.exists(path) else {}
doc["cpu"] = [[fn, args, stated_bytes(capi, fn, args)] for fn, args in CPU_CASES]
with open(path, "w") as f:
    f.write("{\n" + ",\n".join(' "%s": [\n  %s\n ]' % (k, ",\n  ".join(json.dumps(c) for c in doc[k])) for k in sorted(doc)) + "\n}\n")
print(path, {k: len(v) for k, v in doc.items()})
