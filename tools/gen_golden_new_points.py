"""Generate tests/golden/new_points_ref.npz from the REAL reference LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:309-540, with ComputeF12
:1141-1157 and SkewSymmetricMatrix :1287-1291), ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:661-827) and KeyFrame::UnprojectStereo
(src/KeyFrame.cc:720-736).  ORBmatcher.cc and the other whole files are compiled where they lie against oracle/shim, as oracle/Makefile's ref_match
recipe does; the line ranges are extracted into a temporary directory (nothing extracted is kept) and compiled, unedited, with
tools/new_points_golden/new_points_standins.hpp force-included, which supplies what the shim lacks.  Inputs are regenerated from seeds by
tests/new_points_cases.py; only outputs are stored.  The stereo-parallax cosine is computed by the reference itself.
    python tools/gen_golden_new_points.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import new_points_cases as NC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")
GD = os.path.join(ROOT, "tools", "new_points_golden")
RANGES = (("src/LocalMapping.cc", ((309, 540), (1141, 1157), (1287, 1291))), ("src/KeyFrame.cc", ((720, 736),)))


def build(tmp):
    subprocess.check_call(["make", "-C", OR, f"REF={REF}", "_ref/gen/frame_extract_match.cpp"])
    ext = os.path.join(tmp, "new_points_extract.cpp")
    with open(ext, "w") as f:
        f.write("namespace Planar_SLAM {\n")
        for rel, ranges in RANGES:
            lines = open(os.path.join(REF, rel), encoding="utf-8", errors="replace").read().split("\n")
            for a, b in ranges:
                f.write("\n".join(lines[a - 1:b]) + "\n")
        f.write("}\n#include \"ref_new_points_main.cpp\"\n")
    flags = ["-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_ALGEBRA", "-DSTANDINS_REAL_FRAME_FUNCS", f"-I{OR}/shim", f"-I{REF}", f"-I{REF}/include", f"-I{GD}"]
    objs = []
    for i, src in enumerate([f"{OR}/cvprim.cpp", f"{OR}/_ref/gen/frame_extract_match.cpp", f"{REF}/src/ORBmatcher.cc", f"{REF}/src/LSDmatcher.cpp",
                             f"{REF}/src/PlaneMatcher.cpp", f"{REF}/Thirdparty/DBoW2/DBoW2/FeatureVector.cpp"]):
        objs.append(os.path.join(tmp, f"ref{i}.o"))
        subprocess.check_call(["g++"] + flags + ["-include", f"{OR}/shim/match_standins.hpp", "-c", "-o", objs[-1], src], cwd=OR)
    objs.append(os.path.join(tmp, "extract.o"))
    subprocess.check_call(["g++"] + flags + ["-include", f"{GD}/new_points_standins.hpp", "-c", "-o", objs[-1], ext], cwd=OR)
    exe = os.path.join(tmp, "ref_new_points")
    subprocess.check_call(["g++", "-o", exe] + objs)
    return exe


def run(exe, tmp, blocks):
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    NC.write_blocks(pin, blocks)
    subprocess.check_call([exe, pin, pout])
    return NC.read_blocks(pout)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, args in NC.CASES:
            cam, cur, neigh, nn = NC.new_points_case(**args)
            B, S, K = cur["keys_un"].shape[0], cur["keys_un"].shape[1], args["K"]
            n_new = np.zeros(B, np.int32); tri = np.full((B, S, 3), -1, np.int32); x = np.zeros((B, S, 3), np.float32)
            for b in range(B):
                blocks = NC.create_blocks(cam, cur, neigh, nn, K, b)
                r = run(exe, tmp, blocks)
                m = int(np.frombuffer(r[0], np.int32)[0])
                n_new[b] = m; tri[b, :m] = np.frombuffer(r[1], np.int32).reshape(m, 3); x[b, :m] = np.frombuffer(r[2], np.float32).reshape(m, 3)
            out[name + "_n_new"] = n_new; out[name + "_triples"] = tri; out[name + "_x3d"] = x
            print(name, "n_new", n_new.tolist())
        for name, args, only_stereo, ori in NC.PAIR_CASES:
            cam, cur, neigh, nn = NC.new_points_case(**args)
            B, S = cur["keys_un"].shape
            m = np.full((B, S), -1, np.int32); nm = np.zeros(B, np.int32)
            for b in range(B):
                r = run(exe, tmp, [np.array([1, 1, int(only_stereo), int(ori)], np.int32), NC.cam_block(cam)] + NC.kf_blocks(cur, b) + NC.kf_blocks(neigh, b))
                mb = np.frombuffer(r[0], np.int32)
                m[b, :len(mb)] = mb; nm[b] = int(np.frombuffer(r[1], np.int32)[0])
            out[name + "_match"] = m; out[name + "_n"] = nm
            print(name, "nmatches", nm.tolist())
    dst = os.path.join(ROOT, "tests", "golden", "new_points_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
