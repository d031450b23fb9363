"""Generate tests/golden/kf_proj_ref.npz from the REAL reference ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
(src/ORBmatcher.cc:1537-1663): tools/kf_proj_golden/ref_kf_proj_main.cpp is compiled with the reference's ORBmatcher.cc where it lies, against the
stand-ins of oracle/shim, exactly as oracle/Makefile's ref_match recipe compiles it.  Inputs are regenerated from seeds by tests/kf_search_cases.py;
only outputs are stored.
    python tools/gen_golden_kf_proj.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import kf_search_cases as KC  # noqa: E402
from planarslam_amd import guided  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")


def build(tmp):
    subprocess.check_call(["make", "-C", OR, f"REF={REF}", "_ref/gen/frame_extract_match.cpp"])
    exe = os.path.join(tmp, "ref_kf_proj")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_ALGEBRA", "-DSTANDINS_REAL_FRAME_FUNCS", f"-I{OR}/shim", f"-I{REF}",
                           f"-I{REF}/include", "-include", f"{OR}/shim/match_standins.hpp", "-o", exe,
                           os.path.join(ROOT, "tools", "kf_proj_golden", "ref_kf_proj_main.cpp"), f"{OR}/cvprim.cpp", f"{OR}/_ref/gen/frame_extract_match.cpp",
                           f"{REF}/src/ORBmatcher.cc", f"{REF}/src/LSDmatcher.cpp", f"{REF}/src/PlaneMatcher.cpp", f"{REF}/Thirdparty/DBoW2/DBoW2/FeatureVector.cpp"],
                          cwd=OR)
    return exe


def run_pair(exe, tmp, cur, kf, b, th, orb, ori, lsf=None):
    fv, _ = guided.frame_view(cur)
    n, np_ = int(cur["n"][b]), int(kf["n"][b])
    intr = np.array([fv.min_x, fv.max_x, fv.min_y, fv.max_y, fv.grid_w_inv, fv.grid_h_inv, fv.fx, fv.fy, fv.cx, fv.cy], np.float32)
    blocks = [np.array([th, orb, float(ori), KC.log_scale_factor(cur) if lsf is None else lsf, len(cur["scale_factors"])], np.float32),
              np.ascontiguousarray(cur["keys_un"][b, :n]), cur["desc"][b, :n], cur["blocked"][b, :n].astype(np.uint8), intr,
              np.asarray(cur["scale_factors"], np.float32), np.asarray(cur["Tcw"][b], np.float32),
              kf["usable"][b, :np_].astype(np.uint8), kf["found"][b, :np_].astype(np.uint8), kf["xw"][b, :np_].astype(np.float32),
              kf["min_dist"][b, :np_].astype(np.float32), kf["max_dist"][b, :np_].astype(np.float32), kf["angle"][b, :np_].astype(np.float32), kf["desc"][b, :np_]]
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(pin, "wb") as f:
        for a in blocks:
            raw = np.ascontiguousarray(a).tobytes()
            f.write(np.int64(len(raw)).tobytes()); f.write(raw)
    subprocess.check_call([exe, pin, pout])
    raw = open(pout, "rb").read()
    k = int(np.frombuffer(raw[:8], np.int64)[0])
    match = np.frombuffer(raw[8:8 + k], np.int32)
    nm = int(np.frombuffer(raw[16 + k:20 + k], np.int32)[0])
    return match, nm


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, args, th, orb, ori in KC.CASES:
            cur, kf = KC.kf_case(**args)
            B, S = cur["keys_un"].shape
            m = np.full((B, S), -1, np.int32); nm = np.zeros(B, np.int32)
            for b in range(B):
                mb, nb = run_pair(exe, tmp, cur, kf, b, th, orb, ori)
                m[b, :len(mb)] = mb; nm[b] = nb
            out[name + "_match"] = m; out[name + "_n"] = nm
            print(name, "nmatches", nm.tolist(), "matched keypoints", (m >= 0).sum(1).tolist())
    dst = os.path.join(ROOT, "tests", "golden", "kf_proj_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
