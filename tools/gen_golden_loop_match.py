"""Generate tests/golden/loop_match_ref.npz from the REAL reference's four loop-closing matchers, ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*) (src/ORBmatcher.cc:526-659),
SearchBySim3 (:1106-1330), SearchByProjection(KeyFrame*, Scw, ...) (:294-407) and Fuse(KeyFrame*, Scw, ...) (:981-1104):
tools/loop_match_golden/ref_loop_match_main.cpp is compiled with the reference's ORBmatcher.cc where it lies, exactly as tools/gen_golden_kf_proj.py compiles it,
but against tools/loop_match_golden/loop_match_standins.hpp, whose MapPoint::GetIndexInKeyFrame, KeyFrame::GetMapPoints and KeyFrame::AddMapPoint store and answer
for real.  The extracted KeyFrame / MapPoint bodies come from `make -C oracle _ref/gen/frame_extract_match.cpp`.  Inputs are regenerated from seeds by
tests/loop_match_cases.py; only outputs are stored.  A second run reproduces the file byte for byte (fixed zip timestamps).
    python tools/gen_golden_loop_match.py [/path/to/reference]"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import loop_match_cases as LC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")
HERE = os.path.join(ROOT, "tools", "loop_match_golden")


def build(tmp):
    subprocess.check_call(["make", "-C", OR, f"REF={REF}", "_ref/gen/frame_extract_match.cpp"])
    exe = os.path.join(tmp, "ref_loop_match")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_ALGEBRA", "-DSTANDINS_REAL_FRAME_FUNCS", f"-I{OR}/shim", f"-I{REF}",
                           f"-I{REF}/include", "-include", os.path.join(HERE, "loop_match_standins.hpp"), "-o", exe, os.path.join(HERE, "ref_loop_match_main.cpp"),
                           f"{OR}/cvprim.cpp", f"{OR}/_ref/gen/frame_extract_match.cpp", f"{REF}/src/ORBmatcher.cc", f"{REF}/src/LSDmatcher.cpp",
                           f"{REF}/src/PlaneMatcher.cpp", f"{REF}/Thirdparty/DBoW2/DBoW2/FeatureVector.cpp"], cwd=OR)
    return exe


def call(exe, tmp, mode, blocks):
    """-> the blocks the driver wrote, as bytes"""
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    LC.write_blocks(pin, blocks)
    subprocess.check_call([exe, mode, pin, pout])
    return LC.read_blocks(pout)


def run_sim3(exe, tmp, case, b, th):
    m, nf = call(exe, tmp, "sim3", LC.sim3_blocks(case, b, th))
    return np.frombuffer(m, np.int32), int(np.frombuffer(nf, np.int32)[0])


def run_bow(exe, tmp, case, b, nn_ratio, ori):
    m, nm = call(exe, tmp, "bow", LC.bow_blocks(case, b, nn_ratio, ori))
    return np.frombuffer(m, np.int32), int(np.frombuffer(nm, np.int32)[0])


def run_proj(exe, tmp, case, b, th):
    m, nm = call(exe, tmp, "proj", LC.proj_blocks(case, b, th))
    return np.frombuffer(m, np.int32), int(np.frombuffer(nm, np.int32)[0])


def run_fuse(exe, tmp, case, b, th):
    idx, owner, slots, nf = call(exe, tmp, "fuse", LC.fuse_blocks(case, b, th))
    return np.frombuffer(idx, np.int32), np.frombuffer(owner, np.int32), np.frombuffer(slots, np.int32), int(np.frombuffer(nf, np.int32)[0])


def save_reproducible(dst, arrays):
    """np.savez_compressed with a fixed member order and timestamp"""
    with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, args, th in LC.SIM3_CASES:
            case = LC.sim3_case(**args)
            B, S = case["match12"].shape
            m = case["match12"].copy(); nf = np.zeros(B, np.int32)
            for b in range(B):
                mb, nf[b] = run_sim3(exe, tmp, case, b, th)
                m[b, :len(mb)] = mb
            out[name + "_match12"] = m.astype(np.int16); out[name + "_n_found"] = nf
            print(name, "n_found", nf.tolist())
        for name, args, nn_ratio, ori in LC.BOW_CASES:
            case = LC.bow_case(**args)
            B, S = case["node1"].shape
            m = np.full((B, S), -1, np.int32); nm = np.zeros(B, np.int32)
            for b in range(B):
                mb, nm[b] = run_bow(exe, tmp, case, b, nn_ratio, ori)
                m[b, :len(mb)] = mb
            out[name + "_match12"] = m.astype(np.int16); out[name + "_nmatches"] = nm
            print(name, "nmatches", nm.tolist())
        for name, args, th, fuse_th in LC.SCW_CASES:
            case = LC.scw_case(**args)
            B, S = case["kf"]["keys_un"].shape
            PS = case["usable_b"].shape[1]
            m = np.full((B, S), -1, np.int32); nm = np.zeros(B, np.int32)
            fi = np.full((B, PS), -9, np.int32); ow = np.full((B, PS), -9, np.int32); sl = np.full((B, S), -1, np.int32); nf = np.zeros(B, np.int32)
            for b in range(B):
                mb, nm[b] = run_proj(exe, tmp, case, b, th)
                m[b, :len(mb)] = mb
                ib, ob, sb, nf[b] = run_fuse(exe, tmp, case, b, fuse_th)
                fi[b, :len(ib)] = ib; ow[b, :len(ob)] = ob; sl[b, :len(sb)] = sb
            out[name + "_kf_match"] = m.astype(np.int16); out[name + "_nmatches"] = nm
            out[name + "_fuse_idx"] = fi.astype(np.int16); out[name + "_owner"] = ow.astype(np.int16); out[name + "_slots"] = sl.astype(np.int16); out[name + "_n_fused"] = nf
            print(name, "nmatches", nm.tolist(), "n_fused", nf.tolist())
    save_reproducible(LC.GOLDEN_PATH, out)
    print("wrote", LC.GOLDEN_PATH, os.path.getsize(LC.GOLDEN_PATH), "bytes")


if __name__ == "__main__":
    main()
