"""tests/golden/line3d_ref.npz and line3d_edges_ref.npz: what the REAL reference's Frame::isLineGood (oracle/_ref/ref_line3d: src/Frame.cc:189-267 +
src/LineExtractor.cpp helpers extracted by line range, srand(seed + i) before line i) returns on the seeded cases of tests/line3d_cases.py.

    python tools/gen_golden_line3d.py [scenes] [edges]      (no argument: both files)

`scenes` are the detected key lines of CASES, `edges` the hand-built ones of EDGE_CASES (never the sub-pixel line: the reference indexes the image with int(NaN) on it)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import line3d_cases as cases  # noqa: E402
import oracle_lib as O  # noqa: E402


def generate(names, build, dst):
    out = {}
    for name in names:
        kl, d, seed = build(name)
        r = O.run_ref_line3d(kl, d, seed)
        for k, v in r.items():
            out[f"{name}/{k}"] = v
        print(name, len(kl), "lines,", int(r["good"].sum()), "good, inliers", r["n_inliers"][r["good"] > 0][:8])
    path = os.path.join(ROOT, "tests", "golden", dst)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


which = sys.argv[1:] or ["scenes", "edges"]
if "scenes" in which:
    generate(cases.CASES, cases.build, "line3d_ref.npz")
if "edges" in which:
    generate(cases.EDGE_CASES, cases.build_edge, "line3d_edges_ref.npz")
