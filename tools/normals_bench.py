"""normals_kernel alone on the device: B frames (16 synthetic depth images, repeated), one launch at a time between two events on the launch's own stream.
Prints one JSON line: the per-launch times, their median and spread, and a digest of every normal.

    python tools/normals_bench.py [B=2048] [launches=7]
    PLANAR_HIP_LIB=planarslam_amd/libplanar_hip_parent.so python tools/normals_bench.py      # another build of the library on the same frames

Two builds compute the same normals when their digests are equal."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from planarslam_amd import synth
from planarslam_amd._lib import Context
from planarslam_amd.planes import SurfaceNormals

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
REPS = max(5, int(sys.argv[2]) if len(sys.argv) > 2 else 7)
DISTINCT = 16

d = np.stack([synth.depth_image(60 + i, noise=(i % 2 == 0), holes=(i % 3 != 0)) for i in range(DISTINCT)])
d = np.concatenate([d] * (-(-B // DISTINCT)))[:B]
ctx = Context(0)
stream = torch.cuda.Stream()                       # a stream of its own: the launches and the events that time them are on it
ctx.set_stream(stream.cuda_stream)
torch.cuda.set_stream(stream)
sn = SurfaceNormals(640, 480, B, ctx)
dd = torch.from_numpy(d.view(np.int16)).cuda()
out = torch.zeros((B, sn.count, 3), dtype=torch.float32, device="cuda")
for _ in range(2):                                  # warm-up: code object, workspace
    sn.compute_dev(dd.data_ptr(), out.data_ptr(), B)
torch.cuda.synchronize()
ms = []
for _ in range(REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sn.compute_dev(dd.data_ptr(), out.data_ptr(), B)
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
v = np.asarray(ms)
print(json.dumps(dict(tool="normals_bench", lib=os.environ.get("PLANAR_HIP_LIB", "libplanar_hip.so"), B=B, launches=REPS, median_ms=round(float(np.median(v)), 4),
                      min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4), spread_ms=round(float(v.max() - v.min()), 4), all_ms=[round(float(x), 4) for x in v],
                      digest=hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest())))
