"""Generate tests/golden/sim3_opt_ref.npz from the REAL Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3739-3934): `make -C oracle _ref/ref_opt` compiles the
reference's Optimizer.cc, Converter.cc, types_seven_dof_expmap.cpp and its vendored g2o into oracle/_ref/obj_opt; tools/sim3_opt_golden/ref_sim3_opt_main.cpp is
compiled with the same flags and linked against those objects in place of that program's main.o.  Inputs are regenerated from seeds by tests/sim3_opt_cases.py; only
outputs are stored: S12 as the bits of its doubles, match12 as int16, n_inliers.  A second run reproduces the file byte for byte (fixed zip timestamps).
    python tools/gen_golden_sim3_opt.py [/path/to/reference]"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import loop_match_cases as LC  # noqa: E402
import sim3_opt_cases as SC  # noqa: E402
from gen_golden_loop_match import save_reproducible  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")
HERE = os.path.join(ROOT, "tools", "sim3_opt_golden")


def build(tmp):
    subprocess.check_call(["make", "-C", OR, f"REF={REF}", "_ref/ref_opt"])
    objs = sorted(o for o in glob.glob(os.path.join(OR, "_ref", "obj_opt", "*.o")) if os.path.basename(o) != "main.o")
    exe = os.path.join(tmp, "ref_sim3_opt")
    flags = ["-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_ALGEBRA", "-Ishim/minieigen", "-Ishim", f"-I{REF}", f"-I{REF}/include", f"-I{REF}/Thirdparty/g2o"]
    subprocess.check_call(["g++"] + flags + ["-include", "shim/opt_standins.hpp", "-o", exe, os.path.join(HERE, "ref_sim3_opt_main.cpp")] + objs + ["cvprim.cpp"], cwd=OR)
    return exe


def run_pair(exe, tmp, case, b):
    """-> (match12 [n1] on exit, nIn, S12 [8])"""
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    LC.write_blocks(pin, SC.pair_blocks(case, b))
    subprocess.check_call([exe, pin, pout])
    m, nin, S = LC.read_blocks(pout)
    return np.frombuffer(m, np.int32), int(np.frombuffer(nin, np.int32)[0]), np.frombuffer(S, np.float64)


def run_case(exe, tmp, case):
    B = case["match12"].shape[0]
    m = case["match12"].copy(); nin = np.zeros(B, np.int32); S = np.zeros((B, 8))
    for b in range(B):
        mb, nin[b], S[b] = run_pair(exe, tmp, case, b)
        m[b, :len(mb)] = mb
    return m, nin, S


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, args in SC.CASES:
            case = SC.opt_case(**args)
            m, nin, S = run_case(exe, tmp, case)
            again = run_case(exe, tmp, case)
            assert (again[0] == m).all() and (again[1] == nin).all() and again[2].tobytes() == S.tobytes(), "the reference does not repeat itself"
            assert np.abs(m).max() < 32768
            out[name + "_match12"] = m.astype(np.int16); out[name + "_n_inliers"] = nin; out[name + "_S12_bits"] = S.view(np.uint64)
            print(name, "n_inliers", nin.tolist(), "cleared", [int(((case["match12"][b] != -1) & (m[b] == -1)).sum()) for b in range(len(nin))])
    save_reproducible(SC.GOLDEN_PATH, out)
    print("wrote", SC.GOLDEN_PATH, os.path.getsize(SC.GOLDEN_PATH), "bytes")


if __name__ == "__main__":
    main()
