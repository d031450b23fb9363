"""Where lsd_detect's cycles go on the frames bench.py times: B SE3 camera streams (planarslam_amd/synth_se3.py, the bench's seeds), the line extractor in the
bench's top-lines mode, lsd_detect alone on the device (planar_lsd_set_profiling events).  Prints the kernel's own cycle counters (Misc::t: total, region_grow,
region2rect, refine) as mean cycles per frame with n_regions / n_grown_px, the alone time per launch and a digest of the key lines, descriptors and line equations.

    python tools/lsd_detect_split.py [B=2048] [reps=5] [canvases=256] [procs=16]      # procs = 1 under rocprofv3 --pmc (it hangs when the profiled process forks)
    PLANAR_HIP_LIB=planarslam_amd/libplanar_hip_parent.so python tools/lsd_detect_split.py      # another build of the library on the same frames

Two builds compute the same lines when their digests are equal."""
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

from planarslam_amd import synth_se3
from planarslam_amd._lib import KEYLINE_DTYPE, Context, check, lib
from planarslam_amd.lines import LineSegment

dev = torch.device("cuda:0")
ctx = Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
K = 2
loop_g, _, _ = synth_se3.render_streams(torch, torch.from_numpy(canv_g).to(dev), B, K, TUM3, seed=0, W=W, H=H)
ls = LineSegment(W, H, B, ctx, top_only=True)
kl = torch.zeros(B * LINES * KEYLINE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
desc = torch.zeros(B * LINES * 32, dtype=torch.uint8, device=dev)
eq = torch.zeros(B * LINES * 3, dtype=torch.float64, device=dev)
n = torch.zeros(B, dtype=torch.int32, device=dev)
L = lib()


def run(j):
    g = loop_g[:, j].contiguous()
    check(L.planar_lsd_extract_dev(ls.h, g.data_ptr(), B, W, W * H, LINES, kl.data_ptr(), desc.data_ptr(), eq.data_ptr(), n.data_ptr()))
    torch.cuda.synchronize()
    check(L.planar_lsd_check(ls.h, B))


for j in range(K):                                 # warm-up: code objects, workspaces
    run(j)
ms = []
digest = hashlib.sha256()
check(L.planar_lsd_set_profiling(ls.h, 1))
for r in range(REPS):
    for j in range(K):
        run(j)
        tot = (C.c_double * 4)(); calls = C.c_int64()
        check(L.planar_lsd_get_profile(ls.h, tot, C.byref(calls)))
        ms.append((j, [tot[i] / max(1, calls.value) for i in range(4)]))
        if r == 0:
            nn = n.cpu().numpy()
            klh = kl.cpu().numpy().reshape(B, LINES, -1); dh = desc.cpu().numpy().reshape(B, LINES, 32); eh = eq.cpu().numpy().reshape(B, LINES, 3)
            digest.update(nn.tobytes())
            for b in range(B):
                digest.update(klh[b, :nn[b]].tobytes()); digest.update(dh[b, :nn[b]].tobytes()); digest.update(eh[b, :nn[b]].tobytes())
check(L.planar_lsd_set_profiling(ls.h, 0))
run(0)
t = np.stack([ls.read_stage(b, 5) for b in range(B)]).astype(np.float64)          # frame 0 of every stream
regions = np.array([int(ls.read_stage(b, 4)[0]) for b in range(B)], np.float64)
det = np.array([m[2] for _, m in ms])
out = dict(tool="lsd_detect_split", lib=os.environ.get("PLANAR_HIP_LIB", "libplanar_hip.so"), B=B, reps=REPS, frames_per_stream=K,
           lsd_detect_alone_ms=dict(min=float(det.min()), median=float(np.median(det)), max=float(det.max()), all=[round(float(x), 3) for x in det]),
           stage_ms_median=dict(zip(("preprocess", "lsd_sort", "lsd_detect", "rest"), [float(np.median([m[i] for _, m in ms])) for i in range(4)])),
           cycles_per_frame_mean=dict(total=t[:, 0].mean(), region_grow=t[:, 1].mean(), region2rect=t[:, 2].mean(), refine=t[:, 3].mean(),
                                      seed_scan_and_rest=(t[:, 0] - t[:, 1] - t[:, 2] - t[:, 3]).mean()),
           cycles_per_frame_max=dict(total=t[:, 0].max(), region_grow=t[:, 1].max(), region2rect=t[:, 2].max(), refine=t[:, 3].max()),
           n_ord_mean=t[:, 5].mean(), n_regions_mean=regions.mean(), n_grown_px_mean=t[:, 6].mean(), lines_mean=float(n.float().mean()),
           digest=digest.hexdigest())
print(json.dumps(out))
