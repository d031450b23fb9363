"""The two descriptor kernels alone on the device, on the frames bench.py times: B SE3 camera streams (planarslam_amd/synth_se3.py, the bench's seeds) through
the ORB extractor and the line extractor (top-lines mode), one call at a time with a device synchronisation after each.  Prints one JSON line: the ORB extractor's
per-launch events (`orb_describe` has a slot of its own), the line extractor's four profile slots (lbd_describe is the largest part of the last one; its own
duration comes from running this tool under `rocprofv3 --kernel-trace --stats`), and a digest of every key point, key line and descriptor.

    python tools/descriptor_alone.py [B=2048] [reps=5] [canvases=256] [procs=16]      # procs = 1 under rocprofv3 --pmc (it hangs when the profiled process forks)
    PLANAR_HIP_LIB=planarslam_amd/libplanar_hip_parent.so python tools/descriptor_alone.py      # another build of the library on the same frames

Two builds compute the same features when their digests are equal."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C

import numpy as np

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
NCANV = int(sys.argv[3]) if len(sys.argv) > 3 else 256
PROCS = int(sys.argv[4]) if len(sys.argv) > 4 else 16
W, H, MARGIN, LINES = 640, 480, 48, 40

from planarslam_amd.synth import TUM3, stream_canvases

canv_g, _ = stream_canvases(min(NCANV, B), 0, W + 2 * MARGIN, H + 2 * MARGIN, procs=PROCS)   # before the GPU runtime starts (fork)

import torch

from planarslam_amd import ORBextractor, synth_se3
from planarslam_amd._lib import KEYLINE_DTYPE, KP_DTYPE, Context, check, lib
from planarslam_amd.lines import LineSegment

dev = torch.device("cuda:0")
ctx = Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
K = 2
loop_g, _, _ = synth_se3.render_streams(torch, torch.from_numpy(canv_g).to(dev), B, K, TUM3, seed=0, W=W, H=H)
L = lib()
ls = LineSegment(W, H, B, ctx, top_only=True)
kl = torch.zeros(B * LINES * KEYLINE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
ldesc = torch.zeros(B * LINES * 32, dtype=torch.uint8, device=dev)
eq = torch.zeros(B * LINES * 3, dtype=torch.float64, device=dev)
nl = torch.zeros(B, dtype=torch.int32, device=dev)
ex = ORBextractor(1000, 1.2, 8, 20, 7, width=W, height=H, max_batch=B, ctx=ctx)
cap = ex.kp_cap
kps = torch.zeros(B * cap * KP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
odesc = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)
nk = torch.zeros(B, dtype=torch.int32, device=dev)


def run(j):
    g = loop_g[:, j].contiguous()
    ex.extract_dev(g.data_ptr(), kps.data_ptr(), odesc.data_ptr(), nk.data_ptr(), B)
    torch.cuda.synchronize()
    check(L.planar_orb_check(ex.h))
    check(L.planar_lsd_extract_dev(ls.h, g.data_ptr(), B, W, W * H, LINES, kl.data_ptr(), ldesc.data_ptr(), eq.data_ptr(), nl.data_ptr()))
    torch.cuda.synchronize()
    check(L.planar_lsd_check(ls.h, B))


for j in range(K):                                 # warm-up: code objects, workspaces
    run(j)
orb_ms, lsd_ms = [], []
digest = hashlib.sha256()
ex.set_profiling(True)
check(L.planar_lsd_set_profiling(ls.h, 1))
for r in range(REPS):
    for j in range(K):
        run(j)
        prof, calls = ex.get_profile()
        orb_ms.append({k: t / max(1, n) for k, (t, n) in prof.items()})
        tot = (C.c_double * 4)(); calls = C.c_int64()
        check(L.planar_lsd_get_profile(ls.h, tot, C.byref(calls)))
        lsd_ms.append([tot[i] / max(1, calls.value) for i in range(4)])
        if r == 0:
            n1, n2 = nk.cpu().numpy(), nl.cpu().numpy()
            kh = kps.cpu().numpy().reshape(B, cap, -1); oh = odesc.cpu().numpy().reshape(B, cap, 32)
            klh = kl.cpu().numpy().reshape(B, LINES, -1); dh = ldesc.cpu().numpy().reshape(B, LINES, 32)
            digest.update(n1.tobytes()); digest.update(n2.tobytes())
            for b in range(B):
                digest.update(kh[b, :n1[b]].tobytes()); digest.update(oh[b, :n1[b]].tobytes())
                digest.update(klh[b, :n2[b]].tobytes()); digest.update(dh[b, :n2[b]].tobytes())
ex.set_profiling(False)
check(L.planar_lsd_set_profiling(ls.h, 0))


def spread(v):
    v = np.asarray(v, np.float64)
    return dict(min=round(float(v.min()), 4), median=round(float(np.median(v)), 4), max=round(float(v.max()), 4), all=[round(float(x), 4) for x in v])


out = dict(tool="descriptor_alone", lib=os.environ.get("PLANAR_HIP_LIB", "libplanar_hip.so"), B=B, reps=REPS, frames_per_stream=K,
           orb_describe_alone_ms=spread([m["orb_describe"] for m in orb_ms]),
           orb_launch_ms_median={k: round(float(np.median([m[k] for m in orb_ms])), 4) for k in orb_ms[0]},
           lsd_rest_slot_alone_ms=spread([m[3] for m in lsd_ms]),
           lsd_slot_ms_median=dict(zip(("preprocess", "lsd_sort", "lsd_detect", "improve+accept+keylines+lbd"), [round(float(np.median([m[i] for m in lsd_ms])), 4) for i in range(4)])),
           keypoints_mean=float(nk.float().mean()), lines_mean=float(nl.float().mean()), digest=digest.hexdigest())
print(json.dumps(out))
