"""Generate tests/golden/local_map_ref.npz from the REAL reference Tracking::SearchLocalPoints (src/Tracking.cc:2287-2330), SearchLocalLines (:2332-2377) and
UpdateLocalMap with UpdateLocalLines / UpdateLocalPoints / UpdateLocalKeyFrames (:2394-2552).  The line ranges are extracted into a temporary directory (nothing
extracted is kept) and compiled, unedited, with tools/local_map_golden/local_map_standins.hpp force-included, which supplies minimal Tracking, Frame, KeyFrame,
MapPoint, MapLine and Map; the driver tools/local_map_golden/ref_local_map_main.cpp lays the key frames out so that pointer order is the case's kf_rank.  Inputs
are regenerated from seeds by tests/local_map_cases.py; only outputs are stored: per frame the local key frames, the reference key frame, the local point and line
ids with their "already seen by this frame" flags, and the frame's matches after the bad ones were nulled.
    python tools/gen_golden_local_map.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import local_map_cases as LC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
GD = os.path.join(ROOT, "tools", "local_map_golden")
RANGES = ((2287, 2330), (2332, 2377), (2394, 2552))


def build(tmp):
    lines = open(os.path.join(REF, "src", "Tracking.cc"), encoding="utf-8", errors="replace").read().split("\n")
    ext = os.path.join(tmp, "local_map_extract.cpp")
    with open(ext, "w") as f:
        f.write("namespace Planar_SLAM {\n")
        for a, b in RANGES:
            f.write("\n".join(lines[a - 1:b]) + "\n")
        f.write("}\n#include \"ref_local_map_main.cpp\"\n")
    exe = os.path.join(tmp, "ref_local_map")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-w", f"-I{GD}", "-include", os.path.join(GD, "local_map_standins.hpp"), "-o", exe, ext])
    return exe


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        for name in LC.NAMES:
            case = LC.make(name)
            for f, F in enumerate(case["frames"]):
                LC.frame_stream(case, f).tofile(pin)
                subprocess.check_call([exe, pin, pout])
                r = np.fromfile(pout, np.int32)
                at = [0]

                def take(n):
                    v = r[at[0]:at[0] + n]; at[0] += n
                    assert len(v) == n
                    return v.copy()
                rec = {}
                rec["local_kf"] = take(int(take(1)[0]))
                ref, ref_frame = take(2)
                assert ref == ref_frame                          # mpReferenceKF and mCurrentFrame.mpReferenceKF are set together (:2549-2550)
                rec["ref_kf"] = np.int32(ref)
                n = int(take(1)[0]); rec["lp"] = take(n); rec["lp_seen"] = take(n)
                n = int(take(1)[0]); rec["ll"] = take(n); rec["ll_seen"] = take(n)
                rec["match"] = take(len(F["match"])); rec["line_match"] = take(len(F["line_match"]))
                assert at[0] == len(r)
                for k, v in rec.items():
                    out[f"{name}/{f}/{k}"] = v
                print(name, f, "local key frames", len(rec["local_kf"]), "ref", int(ref), "points", len(rec["lp"]), "lines", len(rec["ll"]))
    dst = os.path.join(ROOT, "tests", "golden", "local_map_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
