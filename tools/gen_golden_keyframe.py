"""Generate tests/golden/keyframe_ref.npz from the REAL reference lines: the end of Tracking::Track (src/Tracking.cc:1973-2003, :321-336), NeedNewKeyFrame
(:2049-2137), CreateNewKeyFrame (:2139-2285), the head of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:123-157), KeyFrame::TrackedMapPoints
(src/KeyFrame.cc:259-284), MapPoint::AddObservation (src/MapPoint.cc:103-114) and MapLine::AddObservation (src/MapLine.cpp:91-100).  The line ranges are extracted
into a temporary directory (nothing extracted is kept) and compiled, unedited, with tools/keyframe_golden/keyframe_standins.hpp force-included; the three ranges that
are the middle of a function get a function head and a closing brace around them.  The driver tools/keyframe_golden/ref_keyframe_main.cpp lays the key frames out
so that pointer order is the case's kf_rank.  Inputs are regenerated from seeds by tests/keyframe_cases.py; only outputs are stored, per case the int32 array the
driver wrote (tests/keyframe_cases.py::parse_ref reads it).
    python tools/gen_golden_keyframe.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import keyframe_cases as KC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
GD = os.path.join(ROOT, "tools", "keyframe_golden")
# (file, first line, last line, function head for a range cut out of the middle of a function)
RANGES = (("Tracking.cc", 321, 336, "void Tracking::CleanVOMatches()"), ("Tracking.cc", 1973, 2003, "void Tracking::CountInliers()"), ("Tracking.cc", 2049, 2137, None),
          ("Tracking.cc", 2139, 2285, None), ("LocalMapping.cc", 123, 157, "void LocalMapping::ProcessNewKeyFrameHead()"), ("KeyFrame.cc", 259, 284, None),
          ("MapPoint.cc", 103, 114, None), ("MapLine.cpp", 91, 100, None))


def build(tmp):
    ext = os.path.join(tmp, "keyframe_extract.cpp")
    with open(ext, "w") as f:
        f.write("namespace Planar_SLAM {\n")
        for name, a, b, head in RANGES:
            lines = open(os.path.join(REF, "src", name), encoding="utf-8", errors="replace").read().split("\n")
            if head:
                f.write(head + " {\n")
            f.write("\n".join(lines[a - 1:b]) + "\n")
            if head:
                f.write("}\n")
        f.write("}\n#include \"ref_keyframe_main.cpp\"\n")
    exe = os.path.join(tmp, "ref_keyframe")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-w", f"-I{GD}", "-include", os.path.join(GD, "keyframe_standins.hpp"), "-o", exe, ext])
    return exe


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        for name in KC.REF_NAMES:
            case = KC.make(name)
            KC.stream(case).tofile(pin)
            subprocess.run([exe, pin, pout], check=True, stdout=subprocess.DEVNULL)
            out[name] = np.fromfile(pout, np.int32)
            KC.parse_ref(case, out[name])
            print(name, len(out[name]))
    dst = os.path.join(ROOT, "tests", "golden", "keyframe_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
