"""Generate tests/golden/essential_graph_ref.npz from the REAL Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2680-2991): `make -C oracle _ref/ref_opt`
compiles the reference's Optimizer.cc, Converter.cc, types_seven_dof_expmap.cpp and its vendored g2o into oracle/_ref/obj_opt;
tools/essential_graph_golden/ref_essential_graph_main.cpp is compiled with the same flags and linked against those objects in place of that program's main.o.  Inputs
are regenerated from seeds by tests/essential_graph_cases.py; only outputs are stored, as bits: the float32 poses, the points and the lines.  The planes that build leaves are NOT
stored: its cv::Mat stand-in (oracle/shim/cvalgebra.hpp) rebinds `correctedP3Dw.rowRange(0, 3).col(0) = ...` instead of writing through the view as OpenCV does, so every
plane keeps the normal of Mat::eye(4, 1); tests/essential_graph_cases.py restates :2951-2990 in float32 instead.  Every graph
is run a second time with its covisibility lists reversed (summation order only); the largest difference of the two runs is stored next to the outputs and a case
above 1e-6 is refused: a condition on the inputs, not a tolerance on the product.  A second run of this script reproduces the file byte for byte.

The sparse solver of that build is oracle/shim/minieigen/minieigen_sparse.hpp, a restatement (Eigen is absent), so the linear solve is not pinned below that.
    python tools/gen_golden_essential_graph.py [/path/to/reference]"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import essential_graph_cases as EC  # noqa: E402
from gen_golden_loop_match import save_reproducible  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else os.environ.get("PLANAR_REFERENCE", "/root/reference")
OR = os.path.join(ROOT, "oracle")
HERE = os.path.join(ROOT, "tools", "essential_graph_golden")
SELF_LIMIT = 1e-6


def build(tmp):
    subprocess.check_call(["make", "-C", OR, f"REF={REF}", "_ref/ref_opt"])
    objs = sorted(o for o in glob.glob(os.path.join(OR, "_ref", "obj_opt", "*.o")) if os.path.basename(o) != "main.o")
    exe = os.path.join(tmp, "ref_essential_graph")
    flags = ["-O2", "-std=c++14", "-ffp-contract=off", "-w", "-DCVSHIM_ALGEBRA", "-Ishim/minieigen", "-Ishim", f"-I{REF}", f"-I{REF}/include", f"-I{REF}/Thirdparty/g2o"]
    subprocess.check_call(["g++"] + flags + ["-include", "shim/opt_standins.hpp", "-o", exe, os.path.join(HERE, "ref_essential_graph_main.cpp")] + objs + ["cvprim.cpp"],
                          cwd=OR)
    return exe


def run_graph(exe, tmp, g, reverse=False):
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    EC.write_blocks(pin, EC.graph_blocks(g, reverse))
    subprocess.check_call([exe, pin, pout])
    po, pp, pl, ppl = EC.read_blocks(pout)
    return (np.frombuffer(po, np.float32).reshape(-1, 16), np.frombuffer(pp, np.float32).reshape(-1, 3), np.frombuffer(pl, np.float64).reshape(-1, 6),
            np.frombuffer(ppl, np.float32).reshape(-1, 4))


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, _ in EC.CASES:
            for b, g in enumerate(EC.case_graphs(name)):
                r = run_graph(exe, tmp, g)
                again = run_graph(exe, tmp, g)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(r, again)), "the reference does not repeat itself"
                d = EC.largest_difference(run_graph(exe, tmp, g, reverse=True)[:3], r[:3])
                moved = float(np.abs(r[0] - g["poses"]).max())
                print(f"{name}[{b}]: n {g['n']} edges {len(g['edges'])} self-difference {d:.3g} poses moved by up to {moved:.3g}")
                assert d <= SELF_LIMIT, f"{name}[{b}]: the reference differs from itself by {d} under a reordering of its sums"
                k = f"{name}_{b}_"
                out[k + "poses_bits"] = r[0].view(np.uint32); out[k + "points_bits"] = r[1].view(np.uint32)
                out[k + "lines_bits"] = r[2].view(np.uint64)
                out[k + "self_difference"] = np.array([d])
    save_reproducible(EC.GOLDEN_PATH, out)
    print("wrote", EC.GOLDEN_PATH, os.path.getsize(EC.GOLDEN_PATH), "bytes")


if __name__ == "__main__":
    main()
