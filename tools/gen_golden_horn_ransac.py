"""Generate tests/golden/horn_ransac_ref.npz from the REAL Sim3Solver (reference src/Sim3Solver.cc): the file is compiled where it lies, never copied, against
tools/horn_ransac_golden/ (stand-ins for KeyFrame, MapPoint, ORBmatcher.h and DUtils/Random.h, and horn_cv.hpp, the slice of OpenCV 3.4 it uses; why not
oracle/shim's cv::Mat: see horn_cv.hpp) and linked with tools/horn_ransac_golden/ref_horn_ransac_main.cpp into oracle/_ref/ref_horn_ransac.  Inputs are regenerated
from seeds by tests/horn_ransac_cases.py; only what the solver left is stored: flags, counts and state per call, R, t, s as float bits, the inlier count of every
iteration, and err1 / err2 of CheckInliers for every (iteration, correspondence) with the two maxError, from which the margin is asserted: every error is at least
1e-3 maxError away from maxError (a NaN error fails every comparison and needs no margin).  A pair that misses the margin stops the generator: change its seed.
The reference is run twice and the runs compared.  A second generation reproduces the file byte for byte (fixed zip timestamps).
    python tools/gen_golden_horn_ransac.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import horn_ransac_cases as HC  # noqa: E402
import loop_match_cases as LC  # noqa: E402
from gen_golden_loop_match import save_reproducible  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else os.environ.get("PLANAR_REFERENCE", "/root/reference")
HERE = os.path.join(ROOT, "tools", "horn_ransac_golden")
MARGIN = 1e-3


def build():
    out = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "ref_horn_ransac")
    flags = ["-O2", "-std=c++14", "-ffp-contract=off", "-w", f"-I{HERE}", f"-I{REF}", f"-I{REF}/include", "-include", os.path.join(HERE, "standins.hpp")]
    subprocess.check_call(["g++"] + flags + ["-o", exe, os.path.join(HERE, "ref_horn_ransac_main.cpp"), os.path.join(REF, "src", "Sim3Solver.cc")])
    return exe


def run_pair(exe, tmp, case, b):
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    LC.write_blocks(pin, HC.pair_blocks(case, b))
    subprocess.check_call([exe, pin, pout])
    return LC.read_blocks(pout)


def max_its_table(exe, tmp, case):
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    LC.write_blocks(pin, HC.pair_blocks(case, 0))
    subprocess.check_call([exe, "--table", pin, pout])
    return np.frombuffer(LC.read_blocks(pout)[0], np.int32)


def margin_of(err, maxerr):
    """the smallest |err - maxError| / maxError over the finite errors of [its, N, 2] against [N, 2]"""
    if err.size == 0:
        return np.inf
    rel = np.abs(err.astype(np.float64) - maxerr[None].astype(np.float64)) / maxerr[None].astype(np.float64)
    rel = rel[np.isfinite(err)]
    return float(rel.min()) if rel.size else np.inf


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build()
        for name, args in HC.CASES:
            case = HC.pair_case(**args)
            B, S = case["match12"].shape
            nc = len(case["calls"])
            calls = np.zeros((nc, B, 6), np.int32); inl = np.zeros((nc, B, S), np.uint8); est = np.zeros((nc, B, 26), np.float32)
            N = np.zeros(B, np.int32); mi = np.zeros(B, np.int32)
            for b in range(B):
                bl = run_pair(exe, tmp, case, b)
                assert [bytes(x) for x in run_pair(exe, tmp, case, b)] == [bytes(x) for x in bl], "the reference does not repeat itself"
                n1 = int(case["kf1"]["n"][b])
                calls[:, b] = np.frombuffer(bl[0], np.int32).reshape(nc, 6)
                inl[:, b, :n1] = np.frombuffer(bl[1], np.uint8).reshape(nc, n1)
                est[:, b] = np.frombuffer(bl[2], np.float32).reshape(nc, 26)
                N[b], mi[b] = np.frombuffer(bl[3], np.int32)
                counts = np.frombuffer(bl[4], np.int32)
                err = np.frombuffer(bl[5], np.float32).reshape(len(counts), N[b], 2)
                maxerr = np.frombuffer(bl[6], np.float32).reshape(N[b], 2)
                m = margin_of(err, maxerr)
                assert m >= MARGIN, f"{name} pair {b}: an error lies {m:.2e} maxError from maxError: change the pair's seed"
                assert np.array_equal(counts, ((err[:, :, 0] < maxerr[None, :, 0]) & (err[:, :, 1] < maxerr[None, :, 1])).sum(1)), "the stored errors do not give the counts"
                out[f"{name}_counts_{b}"] = counts; out[f"{name}_err_bits_{b}"] = err.view(np.uint32); out[f"{name}_maxerr_bits_{b}"] = maxerr.view(np.uint32)
                print(name, b, "N", N[b], "maxIts", mi[b], "calls", calls[:, b, :5].tolist(), "margin %.2e" % m, "counts", counts[:12].tolist())
            out[name + "_calls"] = calls; out[name + "_inliers"] = inl; out[name + "_est_bits"] = est.view(np.uint32); out[name + "_N"] = N; out[name + "_max_its"] = mi
        out["max_its_table"] = max_its_table(exe, tmp, HC.pair_case(**dict(HC.CASES)["edge_counts"])).astype(np.int16)
    save_reproducible(HC.GOLDEN_PATH, out)
    print("wrote", HC.GOLDEN_PATH, os.path.getsize(HC.GOLDEN_PATH), "bytes")


if __name__ == "__main__":
    main()
