"""The one g++ command of the adapter tests: include/planar_adapters.hpp compiled into a small executable against the OpenCV stand-in of oracle/shim (OpenCV is
not in the test image) and, unless told otherwise, linked against libplanar_hip.so.  Test infrastructure only; every caller keeps the flags it always had."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "adapter_shim")
ORACLE = os.path.join(ROOT, "oracle")
LIB = os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")


def shim_source(name):
    return os.path.join(SHIM, name)


def build_command(out, sources, plain=False, algebra=False, shim=None, standins=None, library=True, flags=()):
    """plain: neither -O1 nor -pthread (the bare compile-and-link test).  algebra: -DCVSHIM_ALGEBRA, the stand-in's cv::Mat arithmetic.
    shim: where tests/adapter_shim goes on the include path, "first" (its ORBmatcher.h ... replace the reference's) or "last"; None leaves it out.
    standins: "match" or "opt", the map classes of oracle/shim/<standins>_standins.hpp force-included with -DSTANDINS_NO_REFERENCE; the optimiser's use the
    mini-Eigen, which must precede oracle/shim, whose <Eigen/Core> is the 3-type stub.  library: link libplanar_hip.so with its rpaths.  flags: anything else."""
    cmd = ["g++"] + ([] if plain else ["-O1"]) + ["-std=c++14", "-w"] + ([] if plain else ["-pthread"]) + list(flags)
    if algebra:
        cmd += ["-DCVSHIM_ALGEBRA"]
    if shim == "first":
        cmd += ["-I" + SHIM]
    cmd += ["-I" + os.path.join(ROOT, "include")]
    if standins == "opt":
        cmd += ["-I" + ORACLE, "-I" + os.path.join(ORACLE, "shim", "minieigen")]
    cmd += ["-I" + os.path.join(ORACLE, "shim")]
    if shim == "last":
        cmd += ["-I" + SHIM]
    if standins:
        cmd += ["-DSTANDINS_NO_REFERENCE", "-include", os.path.join(ORACLE, "shim", standins + "_standins.hpp")]
    cmd += ["-o", out] + list(sources) + [os.path.join(ORACLE, "cvprim.cpp")]
    if library:
        cmd += [LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    return cmd
