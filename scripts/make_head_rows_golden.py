"""Record tests/golden/head_rows_parent_tables.json: digests of the tables that the fused sampler's head-row region must leave
alone (the full 16-row image's head tile and head rows, the compact image's gather table, the cooperative training tables), for
the shapes of tests/head_rows_model.py.  Run it against a build of the commit to record, with that checkout in front of this
one's tests on the path:

    PYTHONPATH=<built checkout of the parent commit>:tests python scripts/make_head_rows_golden.py tests/golden/head_rows_parent_tables.json
"""
import json
import sys

import head_rows_model as HM
import test_cpu_head_rows_layout as TL

out = {}
for (D, H, NB, T), name in zip(HM.GRID, HM.IDS):
    hf, _, _ = TL._handle(D, H, NB, T)
    out[name] = TL.parent_digests(hf)
with open(sys.argv[1], "w") as fh:
    json.dump(out, fh, indent=0, sort_keys=True)
    fh.write("\n")
print(len(out), "cases")
