"""Seeded problems shared by tools/gen_golden_frame.py (which runs the REAL reference function bodies, oracle/_ref/ref_frame, on them and stores
their outputs in tests/golden/frame_ref.npz), tests/test_oracle_frame_ref.py (oracle vs those outputs) and the GPU tests (HIP vs those outputs)."""
from planarslam_amd import synth

# Tracking::TrackManhattanFrame: name -> manhattan_scene kwargs
MANHATTAN_CASES = {
    "three_axes": dict(B=12, seed=31),
    "no_z": dict(B=4, seed=5, drop_axis=2, clutter=0.0),                       # v3 = v1 x v2
    "no_x_small": dict(B=4, seed=6, drop_axis=0, clutter=0.1, n_normals=700, n_lines=7),   # v1 = v3 x v2
    "no_y_tiny": dict(B=3, seed=8, drop_axis=1, n_normals=300, n_lines=3),     # v2 = v1 x v3
    "one_axis_only": dict(B=4, seed=13, drop_axis=(0, 2), clutter=0.0),        # numDirectionFound < 2: the aliased R_cm comes back (Tracking.cc:1066-1074)
    "mostly_clutter": dict(B=4, seed=9, n_normals=300, clutter=0.9),
    "big_tilt": dict(B=4, seed=17, tilt_deg=11.0),
}


def frustum_case():
    fr = synth.guided_frame(B=3, N=1000, seed=121)
    return synth.guided_local_map(fr, seed=122, n_points=4000, n_lines=500)


def frustum_scale():
    import numpy as np
    return float(np.float32(np.log(np.float32(1.2)))), 8       # Frame::mfLogScaleFactor = log(mfScaleFactor) (float), mnScaleLevels


def stereo_case():
    """Keypoints (incl. image-border positions and zero-depth holes), a depth frame and a pose for Frame::ComputeStereoFromRGBD / UnprojectStereo."""
    import numpy as np
    from planarslam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(33)
    B, S = 3, 1100
    depth = np.stack([synth.depth_image(4321 + i) for i in range(B)])
    keys = np.zeros((B, S), KP_DTYPE)
    keys["x"] = rng.uniform(0, 639.99, (B, S)).astype(np.float32); keys["y"] = rng.uniform(0, 479.99, (B, S)).astype(np.float32)
    keys["x"][:, :4] = [0.0, 639.0, 0.49, 638.51]; keys["y"][:, :4] = [0.0, 479.0, 478.51, 0.49]
    keys["octave"] = rng.integers(0, 8, (B, S))
    n = np.array([S, 1000, 37], np.int32)
    Tcw = np.stack([synth._se3(rng, 0.3, rng.normal(0, 0.5, 3)).astype(np.float32).ravel() for _ in range(B)])
    return keys, n, depth, Tcw


# Camera.k1 .. Camera.k3 of the reference's Examples/RGB-D yaml files: TUM1, TUM2, and TUM3 (all zero -> mvKeysUn = mvKeys)
DIST = {"TUM1": ((517.306408, 516.469215, 318.643040, 255.313989), (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)),
        "TUM2": ((520.908620, 521.007327, 325.141442, 249.701764), (0.231222, -0.784899, -0.003257, -0.000105, 0.917205)),
        "TUM3": ((535.4, 539.2, 320.1, 247.6), (0.0, 0.0, 0.0, 0.0, 0.0))}


def undistort_case(seed=35):
    """Keypoints over the whole image incl. its four corners (Frame::ComputeImageBounds runs the same call on them) for Frame::UndistortKeyPoints"""
    import numpy as np
    from planarslam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(seed)
    B, S = 3, 1300
    keys = np.zeros((B, S), KP_DTYPE)
    keys["x"] = rng.uniform(0, 639.99, (B, S)).astype(np.float32); keys["y"] = rng.uniform(0, 479.99, (B, S)).astype(np.float32)
    keys["x"][:, :4] = [0.0, 640.0, 0.0, 640.0]; keys["y"][:, :4] = [0.0, 0.0, 480.0, 480.0]
    for f in ("size", "angle", "response"):
        keys[f] = rng.uniform(0, 300, (B, S)).astype(np.float32)
    keys["octave"] = rng.integers(0, 8, (B, S)); keys["class_id"] = -1
    return keys, np.array([S, 1024, 5], np.int32)


def manhattan_pose_case(n=64, seed=31):
    """Rotation_cm [n,9], MF_can [n,9] (unit-quaternion rotations, a few of them only slightly apart as on consecutive frames) and mTcw [n,16]"""
    import numpy as np
    rng = np.random.default_rng(seed)

    def rot(q):
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).astype(np.float32)
    q0 = rng.normal(size=(n, 4))
    q1 = np.where((np.arange(n) % 2 == 0)[:, None], q0 + rng.normal(scale=0.01, size=(n, 4)), rng.normal(size=(n, 4)))
    T = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n, 1)); T[:, [3, 7, 11]] = rng.normal(size=(n, 3)).astype(np.float32)
    T[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = rot(rng.normal(size=(n, 4)))
    return rot(q0), rot(q1), T


# ---- Tracking::TrackManhattanFrame at the edges of the kernel's staged chain sums (256-element blocks, an eight-wide body and a scalar tail) ----
MANHATTAN_EDGE_SN_STRIDE, MANHATTAN_EDGE_LN_STRIDE = 600, 16
# (n_normals, n_lines): nothing but lines, fewer than eight elements, exactly eight, totals of 255 / 256 / 257 / 513, lines behind a tail
MANHATTAN_EDGE_COUNTS = [(0, 9), (1, 0), (7, 0), (8, 0), (248, 7), (249, 7), (250, 7), (256, 0), (513, 0), (300, 3)]


def _one_frame(sc, n, m):
    import numpy as np
    return dict(R_last=sc["R_last"][0].copy(), normals=np.ascontiguousarray(sc["normals"][0, :n]), lines=np.ascontiguousarray(sc["lines"][0, :m]))


def _manhattan_edge_builders():
    import numpy as np
    out = {}
    for i, (n, m) in enumerate(MANHATTAN_EDGE_COUNTS):
        out[f"n{n}_l{m}"] = lambda i=i, n=n, m=m: _one_frame(synth.manhattan_scene(B=1, seed=140 + i, n_normals=MANHATTAN_EDGE_SN_STRIDE, n_lines=MANHATTAN_EDGE_LN_STRIDE,
                                                                                    clutter=0.1), n, m)

    def poisoned():
        """every 7th normal NaN, every 50th (from index 3) the zero vector, line 5 zero: a zero vector lies in every cone and adds to no sum"""
        fr = _one_frame(synth.manhattan_scene(B=1, seed=77, n_normals=600, n_lines=12, clutter=0.1), 600, 12)
        fr["normals"][::7] = np.nan
        fr["normals"][3::50] = 0
        fr["lines"][5] = 0
        return fr
    out["poisoned"] = poisoned
    out["lines_only_two_axes"] = lambda: _one_frame(synth.manhattan_scene(B=1, seed=78, n_normals=1, n_lines=30, drop_axis=1), 0, 30)
    return out


MANHATTAN_EDGE_CASES = _manhattan_edge_builders()      # name -> () -> dict(R_last [3,3] f32, normals [n,3] f32, lines [m,3] f64): one frame each


def manhattan_edge_batch(names=None, fill=3.25):
    """the edge frames stacked into one ragged batch at strides strictly above every count (the poisoned frame has its own stride and stays out); rows past the
    counts hold non-zero garbage that must not be read.  -> (names, manhattan_scene-like dict)"""
    import numpy as np
    names = list(names or [k for k in MANHATTAN_EDGE_CASES if k not in ("poisoned", "lines_only_two_axes")])
    S, T = MANHATTAN_EDGE_SN_STRIDE, MANHATTAN_EDGE_LN_STRIDE
    B = len(names)
    sc = dict(R_last=np.zeros((B, 3, 3), np.float32), normals=np.full((B, S, 3), fill, np.float32), lines=np.full((B, T, 3), -fill, np.float64),
              n_normals=np.zeros(B, np.int32), n_lines=np.zeros(B, np.int32))
    for b, k in enumerate(names):
        fr = MANHATTAN_EDGE_CASES[k]()
        n, m = len(fr["normals"]), len(fr["lines"])
        assert n < S and m < T
        sc["R_last"][b] = fr["R_last"]; sc["normals"][b, :n] = fr["normals"]; sc["lines"][b, :m] = fr["lines"]; sc["n_normals"][b] = n; sc["n_lines"][b] = m
    # garbage that would be seen: unit vectors along the frame's first axis would join a cone
    sc["normals"][:, :, :] = np.where(np.arange(S)[None, :, None] < sc["n_normals"][:, None, None], sc["normals"], sc["R_last"][:, None, :, 0])
    sc["lines"][:, :, :] = np.where(np.arange(T)[None, :, None] < sc["n_lines"][:, None, None], sc["lines"], sc["R_last"][:, None, :, 0].astype(np.float64))
    return names, sc
