#!/usr/bin/env python3
"""Is the device code of the working tree the same as that of a git revision?

Compiles every planarslam_amd/csrc/*.hip of the revision (default HEAD) and of the working tree to device assembly with the Makefile's
HIPFLAGS plus `--cuda-device-only -S`, and the two test variants of `make paranoid` (peac.hip -DPLANAR_REFINE_PARANOID, lsd.hip
-DPLANAR_TEST_HOOKS) as well, and compares the outputs after dropping the lines that hold `__hip_cuid_` (a random id per compilation).
Prints one line per file; exit status 1 if any differs.  Needs hipcc, no GPU.

    python tools/device_code_diff.py [--rev REV] [-j JOBS] [--keep DIR]
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("planarslam_amd", "csrc")
VARIANTS = [("peac.hip", "-DPLANAR_REFINE_PARANOID"), ("lsd.hip", "-DPLANAR_TEST_HOOKS")]


def makefile_var(text, name):
    return re.search(r"^%s \?= (.*)$" % name, text, re.M).group(1).strip()


def device_asm(tree, src, define, hipcc, flags, out):
    cmd = [hipcc] + flags + ([define] if define else []) + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd, cwd=os.path.join(tree, CSRC))
    with open(out) as f:
        return [line for line in f if "__hip_cuid_" not in line]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--keep", help="write the assembly files here instead of a temporary directory")
    args = ap.parse_args()
    with open(os.path.join(ROOT, CSRC, "Makefile")) as f:
        mk = f.read()
    hipcc = os.environ.get("HIPCC", makefile_var(mk, "HIPCC"))
    flags = makefile_var(mk, "HIPFLAGS").replace("$(ARCH)", makefile_var(mk, "ARCH")).split()
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        base = os.path.join(work, "base")
        os.makedirs(base, exist_ok=True)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", args.rev, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", base], stdin=tar.stdout)
        if tar.wait():
            sys.exit("git archive failed")
        srcs = sorted(set(f for t in (base, ROOT) for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")))
        cases = [(s, "") for s in srcs] + VARIANTS
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            jobs = {}
            for src, define in cases:
                for side, tree in (("base", base), ("new", ROOT)):
                    if os.path.exists(os.path.join(tree, CSRC, src)):
                        out = os.path.join(work, "%s_%s%s.s" % (side, src[:-4], define.replace("-D", "_")))
                        jobs[src, define, side] = pool.submit(device_asm, tree, src, define, hipcc, flags, out)
            bad = 0
            for src, define in cases:
                a, b = jobs.get((src, define, "base")), jobs.get((src, define, "new"))
                if a is None or b is None:
                    verdict = "only in %s" % ("the working tree" if a is None else args.rev)
                else:
                    a, b = a.result(), b.result()
                    verdict = "identical (%d lines)" % len(a) if a == b else "DIFFERENT"
                bad += not verdict.startswith("identical")
                print("%-34s %s" % ((src + " " + define).strip(), verdict))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
