"""Generate tests/golden/connections_ref.npz from the REAL reference KeyFrame::AddConnection / UpdateBestCovisibles (src/KeyFrame.cc:132-166) and
UpdateConnections / AddChild (:298-438).  The line ranges are extracted into a temporary directory (nothing extracted is kept) and compiled, unedited, with
tools/connections_golden/connections_standins.hpp force-included, which supplies minimal KeyFrame and MapPoint; the driver
tools/connections_golden/ref_connections_main.cpp lays the key frames out so that pointer order is the case's kf_rank and calls UpdateConnections on the case's
list in order.  Inputs are regenerated from seeds by tests/connections_cases.py; only outputs are stored: per map the stored weights as (key frame, neighbour,
weight), the ordered lists with their weights, the parents, the first-connection flags and the children added, and per entry the parent it was given.
    python tools/gen_golden_connections.py [/path/to/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import connections_cases as CC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PLANAR_REFERENCE", "/root/reference")
GD = os.path.join(ROOT, "tools", "connections_golden")
RANGES = ((132, 166), (298, 438))


def build(tmp):
    lines = open(os.path.join(REF, "src", "KeyFrame.cc"), encoding="utf-8", errors="replace").read().split("\n")
    ext = os.path.join(tmp, "connections_extract.cpp")
    with open(ext, "w") as f:
        f.write("namespace Planar_SLAM {\n")
        for a, b in RANGES:
            f.write("\n".join(lines[a - 1:b]) + "\n")
        f.write("}\n#include \"ref_connections_main.cpp\"\n")
    exe = os.path.join(tmp, "ref_connections")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-w", f"-I{GD}", "-include", os.path.join(GD, "connections_standins.hpp"), "-o", exe, ext])
    return exe


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        for name in CC.NAMES:
            case = CC.make(name)
            CC.stream(case).tofile(pin)
            subprocess.check_call([exe, pin, pout])
            r = np.fromfile(pout, np.int32)
            at = [0]

            def take(n):
                v = r[at[0]:at[0] + n]; at[0] += n
                assert len(v) == n
                return v.copy()
            for g, M in enumerate(case["maps"]):
                conn, ord_n, ord_kf, ord_w, parent, first, child = [], [], [], [], [], [], []
                for k in range(M["nk"]):
                    n = int(take(1)[0])
                    row = take(2 * n).reshape(n, 2)
                    conn.append(np.concatenate([np.full((n, 1), k, np.int32), row], 1))
                    n = int(take(1)[0]); ord_n.append(n); ord_kf.append(take(n)); ord_w.append(take(n))
                    parent.append(int(take(1)[0])); first.append(int(take(1)[0]))
                    n = int(take(1)[0])
                    child.append(np.stack([np.full(n, k, np.int32), take(n)], 1))
                rec = dict(conn=np.concatenate(conn).astype(np.int32), ord_n=np.asarray(ord_n, np.int32), ord_kf=np.concatenate(ord_kf), ord_w=np.concatenate(ord_w),
                           parent=np.asarray(parent, np.int32), first=np.asarray(first, np.uint8), child=np.concatenate(child).astype(np.int32))
                for k, v in rec.items():
                    out[f"{name}/{g}/{k}"] = v
                print(name, g, "weights", len(rec["conn"]), "listed", int(rec["ord_n"].sum()), "children added", len(rec["child"]))
            out[f"{name}/new_parent"] = take(len(case["entries"]))
            assert at[0] == len(r)
    dst = os.path.join(ROOT, "tests", "golden", "connections_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
