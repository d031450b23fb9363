"""planar_is_line_good_dev (line3d_kernel + the packing of the good directions) alone on the device: B frames of 40 key lines each, the key lines taken from the
line extractor on 16 synthetic frames (repeated, every frame with a seed of its own), one call at a time between two events on the call's own stream.
Prints one JSON line: the per-call times, their median and spread, and a digest of every output.

    python tools/line3d_bench.py [B=2048] [launches=7]
    PLANAR_HIP_LIB=planarslam_amd/libplanar_hip_parent.so python tools/line3d_bench.py      # another build of the library on the same lines

Two builds compute the same 3-D lines when their digests are equal."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from planarslam_amd import synth
from planarslam_amd._lib import KEYLINE_DTYPE, Context, check, lib
from planarslam_amd.lines import LineSegment

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
REPS = max(5, int(sys.argv[2]) if len(sys.argv) > 2 else 7)
DISTINCT, W, H, LINES = 16, 640, 480, 40
CAM = (535.4, 539.2, 320.1, 247.6)

ctx = Context(0)
stream = torch.cuda.Stream()                       # a stream of its own: the launches and the events that time them are on it
ctx.set_stream(stream.cuda_stream)
torch.cuda.set_stream(stream)
gray = np.stack([synth.gray_image(11 + i) for i in range(DISTINCT)])
kl16, _, _, n16 = LineSegment(W, H, DISTINCT, ctx).ExtractLineSegment(gray)
d16 = np.stack([synth.depth_image(111 + i, noise=(i % 2 == 0), holes=(i % 3 != 2)) for i in range(DISTINCT)])
rep = -(-B // DISTINCT)
kl = np.concatenate([kl16] * rep)[:B]; nl = np.concatenate([n16] * rep)[:B].astype(np.int32); d = np.concatenate([d16] * rep)[:B]
seeds = (np.arange(B, dtype=np.uint32) * 64 + 7).astype(np.uint32)

dev = torch.device("cuda:0")
t_kl = torch.from_numpy(np.ascontiguousarray(kl).view(np.uint8).reshape(-1)).to(dev)
t_nl = torch.from_numpy(nl).to(dev); t_d = torch.from_numpy(d.view(np.int16)).to(dev); t_seeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
o = dict(depth_line=torch.zeros(B * LINES, dtype=torch.float32, device=dev), lines3d=torch.zeros(B * LINES * 6, dtype=torch.float64, device=dev),
         good=torch.zeros(B * LINES, dtype=torch.uint8, device=dev), direction=torch.zeros(B * LINES * 3, dtype=torch.float64, device=dev),
         n_inliers=torch.zeros(B * LINES, dtype=torch.int32, device=dev), packed=torch.zeros(B * LINES * 3, dtype=torch.float64, device=dev),
         n_good=torch.zeros(B, dtype=torch.int32, device=dev))
L = lib()
assert kl.dtype == KEYLINE_DTYPE


def run():
    check(L.planar_is_line_good_dev(ctx.h, B, t_kl.data_ptr(), t_nl.data_ptr(), LINES, t_d.data_ptr(), W, H, W, W * H, float(np.float32(1.0 / 5000.0)),
                                    *CAM, t_seeds.data_ptr(), o["depth_line"].data_ptr(), o["lines3d"].data_ptr(), o["good"].data_ptr(), o["direction"].data_ptr(),
                                    o["n_inliers"].data_ptr(), o["packed"].data_ptr(), o["n_good"].data_ptr()))


for _ in range(2):                                  # warm-up: code object
    run()
torch.cuda.synchronize()
ms = []
for _ in range(REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
v = np.asarray(ms)
digest = hashlib.sha256()
for k in ("depth_line", "lines3d", "good", "n_inliers", "n_good"):       # the directions go through hypot(): same library on both sides, so they are compared too
    digest.update(o[k].cpu().numpy().tobytes())
digest.update(o["direction"].cpu().numpy().tobytes())
ni = o["n_inliers"].cpu().numpy()
print(json.dumps(dict(tool="line3d_bench", lib=os.environ.get("PLANAR_HIP_LIB", "libplanar_hip.so"), B=B, lines_per_frame=LINES, launches=REPS,
                      median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4), spread_ms=round(float(v.max() - v.min()), 4),
                      all_ms=[round(float(x), 4) for x in v], lines_mean=float(nl.mean()), good_mean=float(o["n_good"].float().mean()), inliers_mean=float(ni[ni > 0].mean()),
                      digest=digest.hexdigest())))
