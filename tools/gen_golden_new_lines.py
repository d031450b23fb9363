"""Generate tests/golden/new_lines_ref.npz from the REAL reference LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:800-1037), LSDmatcher::SearchForTriangulation and
SearchByDescriptor(KeyFrame*, KeyFrame*) (src/LSDmatcher.cpp, compiled where it lies), KeyFrame::obtain3DLine / AddMapLine / GetMapLine / lineDescriptorMAD
(src/KeyFrame.cc:738-747, 781-785, 852-856, 858-883) and MapLine's constructor and UpdateAverageDir (src/MapLine.cpp:16-29, 320-367).  The line ranges are extracted into a
temporary directory (nothing extracted is kept) and compiled, unedited, against oracle/shim with tools/new_lines_golden/new_lines_standins.hpp force-included, which supplies
what the shim lacks.  Inputs are regenerated from seeds by tests/new_lines_cases.py; only outputs are stored.
    python tools/gen_golden_new_lines.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import new_lines_cases as LC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")
GD = os.path.join(ROOT, "tools", "new_lines_golden")
RANGES = (("src/LocalMapping.cc", ((800, 1037),)), ("src/KeyFrame.cc", ((738, 747), (781, 785), (852, 856), (858, 883))), ("src/MapLine.cpp", ((16, 29), (320, 367))))


def build(tmp):
    subprocess.check_call(["make", "-C", OR, f"REF={REF}", "_ref/gen/frame_extract_match.cpp"])
    ext = os.path.join(tmp, "new_lines_extract.cpp")
    with open(ext, "w") as f:
        f.write("using namespace std;\nusing namespace cv;\nusing namespace cv::line_descriptor;\nusing namespace Eigen;\nnamespace Planar_SLAM {\n")
        for rel, ranges in RANGES:
            lines = open(os.path.join(REF, rel), encoding="utf-8", errors="replace").read().split("\n")
            for a, b in ranges:
                f.write("\n".join(lines[a - 1:b]) + "\n")
        f.write("}\n#include \"ref_new_lines_main.cpp\"\n")
    flags = ["-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_ALGEBRA", "-DSTANDINS_REAL_FRAME_FUNCS", f"-I{OR}/shim", f"-I{REF}", f"-I{REF}/include", f"-I{GD}"]
    objs = []
    for i, src in enumerate([f"{OR}/cvprim.cpp", f"{OR}/_ref/gen/frame_extract_match.cpp", f"{REF}/Thirdparty/DBoW2/DBoW2/FeatureVector.cpp"]):
        objs.append(os.path.join(tmp, f"ref{i}.o"))
        subprocess.check_call(["g++"] + flags + ["-include", f"{OR}/shim/match_standins.hpp", "-c", "-o", objs[-1], src], cwd=OR)
    objs.append(os.path.join(tmp, "lsdmatcher.o"))
    subprocess.check_call(["g++"] + flags + ["-include", f"{GD}/new_lines_standins.hpp", "-c", "-o", objs[-1], f"{REF}/src/LSDmatcher.cpp"], cwd=OR)
    objs.append(os.path.join(tmp, "extract.o"))
    subprocess.check_call(["g++"] + flags + ["-DNEW_LINES_EXTRACT", "-include", f"{GD}/new_lines_standins.hpp", "-c", "-o", objs[-1], ext], cwd=OR)
    exe = os.path.join(tmp, "ref_new_lines")
    subprocess.check_call(["g++", "-pthread", "-o", exe] + objs)   # the extracted bodies lock std::mutex
    return exe


def run(exe, tmp, blocks):
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    LC.write_blocks(pin, blocks)
    subprocess.check_call([exe, pin, pout])
    return LC.read_blocks(pout)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, args in LC.CASES:
            cam, cur, neigh, nn = LC.new_lines_case(**args)
            (B, S), K = cur["ldesc"].shape[:2], args["K"]
            assert all(neigh["n"][b * K + k] <= cur["n"][b] for b in range(B) for k in range(K)), "a neighbour with more lines: the reference would read past mvDepthLine"
            n_new = np.zeros(B, np.int32); tri = np.full((B, S, 3), -1, np.int32); x = np.zeros((B, S, 6))
            m = np.full((B, S), -1, np.int32); nm = np.zeros(B, np.int32); mads = np.zeros((B, 2)); md = np.full((B, S), -1, np.int32); nd = np.zeros(B, np.int32)
            for b in range(B):
                r = run(exe, tmp, LC.create_blocks(cam, cur, neigh, nn, K, b))
                k = int(np.frombuffer(r[0], np.int32)[0])
                n_new[b] = k; tri[b, :k] = np.frombuffer(r[1], np.int32).reshape(k, 3); x[b, :k] = np.frombuffer(r[2], np.float64).reshape(k, 6)
                r = run(exe, tmp, LC.create_blocks(cam, cur, neigh, nn, K, b, mode=1))
                mb = np.frombuffer(r[0], np.int32)
                m[b, :len(mb)] = mb; nm[b] = np.frombuffer(r[1], np.int32)[0]; mads[b] = np.frombuffer(r[2], np.float64)
                db = np.frombuffer(r[3], np.int32)
                md[b, :len(db)] = db; nd[b] = np.frombuffer(r[4], np.int32)[0]
            out.update({name + "_n_new": n_new, name + "_triples": tri, name + "_line": x, name + "_tri_match": m, name + "_tri_n": nm, name + "_mads": mads,
                        name + "_desc_match": md, name + "_desc_n": nd})
            print(name, "n_new", n_new.tolist(), "tri", nm.tolist(), "desc", nd.tolist())
        d = LC.average_dir_case()
        G, S = d["xw6"].shape[:2]
        nrm = np.zeros((G, S, 3)); mn = np.zeros((G, S), np.float32); mx = np.zeros((G, S), np.float32)
        for g in range(G):
            r = run(exe, tmp, LC.average_dir_blocks(d, g))
            k = int(d["n"][g])
            nrm[g, :k] = np.frombuffer(r[0], np.float64).reshape(k, 3); mn[g, :k] = np.frombuffer(r[1], np.float32); mx[g, :k] = np.frombuffer(r[2], np.float32)
        out.update(dir_normal=nrm, dir_min=mn, dir_max=mx)
    dst = os.path.join(ROOT, "tests", "golden", "new_lines_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
