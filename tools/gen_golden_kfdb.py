"""Generate tests/golden/kfdb_ref.npz from the REAL reference: src/KeyFrameDatabase.cc (add / erase / DetectRelocalizationCandidates / DetectLoopCandidates) and the vendored
DBoW2 (TemplatedVocabulary.h, ScoringObject.cpp's L1Scoring::score, ...), all compiled where they lie against oracle/shim, with tools/kfdb_golden/kfdb_standins.hpp
force-included in place of KeyFrame.h / Frame.h and tools/kfdb_golden/ref_kfdb_main.cpp as the driver.  The build happens in a temporary directory; nothing of the reference is
kept.  Inputs are regenerated from seeds by tests/kfdb_cases.py; the fixture stores the recorded score inputs, the outputs and the pair scores.
    python tools/gen_golden_kfdb.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import kfdb_cases as KC  # noqa: E402
from planarslam_amd import synth  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")
GD = os.path.join(ROOT, "tools", "kfdb_golden")
DBOW = os.path.join(REF, "Thirdparty", "DBoW2")


def build(tmp):
    flags = ["-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_FILESTORAGE", "-include", "sstream", "-include", "iostream", f"-I{OR}/shim", f"-I{REF}",
             f"-I{REF}/include", f"-I{GD}"]
    objs = []
    plain = [f"{OR}/cvprim.cpp"] + [f"{DBOW}/DBoW2/{n}.cpp" for n in ("FORB", "BowVector", "FeatureVector", "ScoringObject")] + [f"{DBOW}/DUtils/Random.cpp", f"{DBOW}/DUtils/Timestamp.cpp"]
    for i, src in enumerate(plain + [f"{REF}/src/KeyFrameDatabase.cc", f"{GD}/ref_kfdb_main.cpp"]):
        objs.append(os.path.join(tmp, f"ref{i}.o"))
        extra = [] if src in plain else ["-include", f"{GD}/kfdb_standins.hpp"]
        subprocess.check_call(["g++"] + flags + extra + ["-c", "-o", objs[-1], src], cwd=OR)
    exe = os.path.join(tmp, "ref_kfdb")
    subprocess.check_call(["g++", "-pthread", "-o", exe] + objs)
    return exe


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        voc_txt = os.path.join(tmp, "voc.txt")
        synth.write_vocabulary_text(KC.vocabulary(), voc_txt)
        for name in KC.CASES:
            case = KC.build(name)
            pairs = KC.score_pairs(case)
            pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            KC.write_input(pin, case, pairs)
            subprocess.check_call([exe, voc_txt, pin, pout])
            r = KC.read_output(pout, case, len(pairs))
            out.update({f"{name}_{k}": v for k, v in r.items()})
            print(name, "n_cand", r["n_cand"].tolist(), "n_scored", r["n_scored"].tolist())
    dst = os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
