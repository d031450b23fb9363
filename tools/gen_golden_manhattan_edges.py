"""tests/golden/manhattan_edges_ref.npz: what the REAL reference's Tracking::TrackManhattanFrame (oracle/_ref/ref_frame, src/Tracking.cc:763-1157) returns on the
one-frame edge cases of tests/frame_cases.py (MANHATTAN_EDGE_CASES): rotation and cone membership.  Writes only this file; tests/golden/frame_ref.npz is
tools/gen_golden_frame.py's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_cases as cases  # noqa: E402
import oracle_lib as O  # noqa: E402

out = {}
for name, make in cases.MANHATTAN_EDGE_CASES.items():
    fr = make()
    r = O.run_ref_manhattan(fr["R_last"], fr["normals"], fr["lines"])
    out[f"{name}/R"] = r["R"]; out[f"{name}/member"] = r["member"]
    print(name, len(fr["normals"]), "normals,", len(fr["lines"]), "lines, members per axis", [int(((r["member"] >> a) & 1).sum()) for a in range(3)])
path = os.path.join(ROOT, "tests", "golden", "manhattan_edges_ref.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
