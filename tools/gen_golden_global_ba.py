"""Generate tests/golden/global_ba_ref.npz from the REAL Optimizer::GlobalBundleAdjustemnt (reference src/Optimizer.cc:35-548): `make -C oracle _ref/ref_opt` compiles
the reference's Optimizer.cc, Converter.cc and its vendored g2o into oracle/_ref/obj_opt; tools/global_ba_golden/ref_global_ba_main.cpp is compiled with the same
flags and linked against those objects in place of that program's main.o.  Inputs are regenerated from seeds by tests/global_ba_cases.py; only outputs are stored,
as bits: the float32 poses and the landmarks as the map objects hold them afterwards.  The call is made with nLoopKF = 0, so the results come back through SetPose /
SetWorldPos (the copyTo(rowRange(...)) of the nLoopKF != 0 branch is a view the cv::Mat stand-in of that build is known not to write through).

Every case is run a second time with the key-frame objects allocated in reverse order: the std::map<KeyFrame*, size_t> observation lists then iterate the other way,
which changes the summation order and nothing else.  The largest difference of the two runs is stored next to the outputs and a case above 1e-6 is refused: a
condition on the inputs, not a tolerance on the product.  So is a case with a point or line end less than 0.5 m in front of an observer or a plane with |d| < 0.5.
A landmark without an edge must come back exactly as given.  A second run of this script reproduces the file byte for byte.

The sparse solver of that build is oracle/shim/minieigen/minieigen_sparse.hpp, a restatement (Eigen is absent), so the linear solve is unpinned below it.
    python tools/gen_golden_global_ba.py [/path/to/reference]"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import global_ba_cases as GC  # noqa: E402
from gen_golden_loop_match import save_reproducible  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")
HERE = os.path.join(ROOT, "tools", "global_ba_golden")
SELF_LIMIT = 1e-6


def build(tmp):
    subprocess.check_call(["make", "-C", OR, f"REF={REF}", "_ref/ref_opt"])
    objs = sorted(o for o in glob.glob(os.path.join(OR, "_ref", "obj_opt", "*.o")) if os.path.basename(o) != "main.o")
    exe = os.path.join(tmp, "ref_global_ba")
    flags = ["-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_ALGEBRA", "-Ishim/minieigen", "-Ishim", f"-I{REF}", f"-I{REF}/include", f"-I{REF}/Thirdparty/g2o"]
    subprocess.check_call(["g++"] + flags + ["-include", "shim/opt_standins.hpp", "-o", exe, os.path.join(HERE, "ref_global_ba_main.cpp")] + objs + ["cvprim.cpp"], cwd=OR)
    return exe


def run(exe, tmp, pr, robust, reverse=False):
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    GC.write_blocks(pin, GC.reference_blocks(pr, robust, reverse))
    subprocess.check_call([exe, pin, pout], stdout=subprocess.DEVNULL)
    T, lm = GC.read_blocks(pout)
    return np.frombuffer(T, np.float32).reshape(-1, 16), np.frombuffer(lm, np.float64).reshape(-1, 4)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, (builder, robust) in GC.REF_CASES.items():
            pr = builder()
            depth, dmin = GC.conditions(pr)
            assert depth >= GC.MIN_DEPTH and dmin >= GC.MIN_PLANE_D, f"{name}: depth {depth}, plane distance {dmin}"
            T, lm = run(exe, tmp, pr, robust)
            T2, lm2 = run(exe, tmp, pr, robust)
            assert T.tobytes() == T2.tobytes() and lm.tobytes() == lm2.tobytes(), "the reference does not repeat itself"
            Tr, lmr = run(exe, tmp, pr, robust, reverse=True)
            d = max(GC.differences(pr, Tr, lmr, T, lm))
            inc = GC.included(pr).astype(bool)
            assert np.array_equal(lm[~inc, :3], pr["lm_init"][~inc, :3]), f"{name}: a landmark without an edge moved"
            moved = float(np.abs(T - pr["kf_Tcw"]).max())
            print(f"{name}: key frames {len(T)} landmarks {len(lm)} ({int((~inc).sum())} without an edge) edges {len(pr['e_kf'])} robust {robust} "
                  f"self-difference {d:.3g} poses moved by up to {moved:.3g}")
            assert d <= SELF_LIMIT, f"{name}: the reference differs from itself by {d} under a reordering of its sums"
            out[name + "_kf_Tcw_bits"] = T.view(np.uint32); out[name + "_lm_bits"] = lm.view(np.uint64)
            out[name + "_self_difference"] = np.array([d])
    save_reproducible(GC.GOLDEN_PATH, out)
    print("wrote", GC.GOLDEN_PATH, os.path.getsize(GC.GOLDEN_PATH), "bytes")


if __name__ == "__main__":
    main()
