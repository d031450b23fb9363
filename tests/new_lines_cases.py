"""Cases for LocalMapping::CreateNewMapLines2 / LSDmatcher::SearchForTriangulation / SearchByDescriptor(KF, KF) / MapLine::UpdateAverageDir: a current key
frame and K neighbours observing one synthetic set of 3-D segments from SE3 poses around it.  Seeded; inputs are regenerated, never stored.  What is planted:
  * LBD rows shared per segment with bit noise, clutter lines with random rows (their d1 - d0 falls below the MAD threshold), occupied lines on both sides;
  * depth_line > 0 for a share of the lines with lines3d = the end points in the camera frame, -1 and zeros for the rest (as planar_is_line_good leaves them),
    so both stereo sources occur: the current key frame's own 3-D line, and the neighbour's when only depth_line[idx2] OF THE CURRENT key frame is positive;
  * neighbour 1 closer than mb (the baseline gate); forward- and backward-moving neighbours (depth signs in the second camera, both sides of the scale test);
  * 3-D end points moved behind the camera, pulled along their ray to a few centimetres, or pushed sideways (the depth signs and the reprojection gates of the
    first key frame), key-line end points of the neighbours pushed by several sigma (those of the second), random octaves (the scale test);
  * lines duplicated inside the current key frame (two idx1 taking one idx2)."""
import numpy as np

import new_points_cases as NC
from planarslam_amd._lib import KEYLINE_DTYPE

W, H = NC.W, NC.H
# displacement of neighbour k from the current key frame: (sideways, forward) in metres; mb is about 0.075
MOVES = ((0.30, 0.0), (0.04, 0.0), (0.05, 0.45), (0.10, -0.60), (0.45, 0.1), (0.2, 0.3), (0.35, -0.2), (0.25, 0.0), (0.5, 0.0), (0.15, 0.15))


def _observe(rng, cam, T, P, Q, lm, desc_lm, N, S, p, shove):
    """the lines of one key frame: the segments (P, Q) it sees, clutter up to N lines -> dict of [S] arrays"""
    sf = cam["scale_factors"]
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    Pc, Qc = P @ R.T + t, Q @ R.T + t
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))

    def proj(X):
        return np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    ok = (Pc[:, 2] > 0.3) & (Qc[:, 2] > 0.3)
    up, uq = proj(np.where(ok[:, None], Pc, 1.0)), proj(np.where(ok[:, None], Qc, 1.0))
    for u in (up, uq):
        ok &= (u[:, 0] > 4) & (u[:, 0] < W - 4) & (u[:, 1] > 4) & (u[:, 1] < H - 4)
    idx = np.flatnonzero(ok)
    rng.shuffle(idx)
    idx = idx[:int(N * (1 - p["clutter"]))]
    n_obs, n = len(idx), N
    kl = np.zeros(S, KEYLINE_DTYPE)
    zz = 0.5 * (Pc[idx, 2] + Qc[idx, 2])
    octv = np.clip(np.round(np.log(np.maximum(zz, 0.3) / 1.5) / np.log(1.2)), 0, len(sf) - 1).astype(np.int32)
    off = rng.random(n_obs) < p["octave_off"]
    octv[off] = rng.integers(0, len(sf), int(off.sum()))
    sig = sf[octv].astype(np.float64)
    a = up[idx] + rng.normal(size=(n_obs, 2)) * p["pix"] * sig[:, None]
    b = uq[idx] + rng.normal(size=(n_obs, 2)) * p["pix"] * sig[:, None]
    sh = rng.random(n_obs) < shove                       # one end point of the key line pushed by several sigma
    end = rng.random(n_obs) < 0.5
    push = rng.choice([-1, 1], n_obs) * rng.uniform(4, 12, n_obs) * sig
    a[sh & end, 1] += push[sh & end]; b[sh & ~end, 1] += push[sh & ~end]
    kl["start_x"][:n_obs], kl["start_y"][:n_obs], kl["end_x"][:n_obs], kl["end_y"][:n_obs] = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    kl["octave"][:n_obs] = octv
    desc = np.zeros((S, 32), np.uint8)
    desc[:n_obs] = desc_lm[lm[idx]]
    nb = rng.integers(0, p["bits"] + 1, n_obs)
    flip = rng.random((n_obs, 256)).argsort(1).argsort(1) < nb[:, None]
    desc[:n_obs] ^= np.packbits(flip, axis=1, bitorder="little")
    l3 = np.zeros((S, 6)); dl = np.full(S, -1, np.float32)
    A, Bq = Pc[idx] * (1 + rng.normal(size=(n_obs, 1)) * 0.004), Qc[idx] * (1 + rng.normal(size=(n_obs, 1)) * 0.004)
    bad = rng.random(n_obs) < p["bad3d"]                   # a wrong 3-D end point
    kind = rng.integers(0, 3, n_obs); which = rng.random(n_obs) < 0.5
    for i in np.flatnonzero(bad):
        E = A if which[i] else Bq
        if kind[i] == 0: E[i] = E[i] * -rng.uniform(0.2, 1.0)                       # behind the camera
        elif kind[i] == 1: E[i] = E[i] * (rng.uniform(0.03, 0.25) / E[i, 2])        # on its ray, a few centimetres ahead
        else: E[i, :2] += rng.choice([-1, 1], 2) * rng.uniform(0.08, 0.4, 2)        # beside its ray
    st = rng.random(n_obs) < p["stereo"]
    l3[:n_obs][st] = np.concatenate([A, Bq], 1)[st]
    dl[:n_obs][st] = zz[st].astype(np.float32)
    # clutter: random segments, random rows, no 3-D line
    m = n - n_obs
    ca = np.stack([rng.uniform(10, W - 10, m), rng.uniform(10, H - 10, m)], 1)
    cb = np.clip(ca + rng.normal(size=(m, 2)) * 60, 5, [W - 5, H - 5])
    kl["start_x"][n_obs:n], kl["start_y"][n_obs:n], kl["end_x"][n_obs:n], kl["end_y"][n_obs:n] = ca[:, 0], ca[:, 1], cb[:, 0], cb[:, 1]
    kl["octave"][n_obs:n] = rng.integers(0, len(sf), m)
    desc[n_obs:n] = rng.integers(0, 256, (m, 32))
    lmk = np.full(S, -1, np.int64); lmk[:n_obs] = lm[idx]
    kl["pt_x"] = 0.5 * (kl["start_x"] + kl["end_x"]); kl["pt_y"] = 0.5 * (kl["start_y"] + kl["end_y"])
    kl["class_id"][:n] = np.arange(n)
    occ = np.zeros(S, np.uint8); occ[:n] = rng.random(n) < p["occupied"]
    # a random order, so that observed lines and clutter mix and depth_line[idx2] of the current key frame is unrelated to line idx1
    perm = np.concatenate([rng.permutation(n), np.arange(n, S)])
    return dict(n=n, keylines=kl[perm], ldesc=desc[perm], occupied=occ[perm], depth_line=dl[perm], lines3d=l3[perm], lm=lmk[perm], Tcw=T.reshape(16))


def _duplicate(rng, k, m):
    """overwrite the last m lines with copies of observed ones, a fraction of a pixel away: equal rows"""
    n = k["n"]
    src = rng.choice(np.flatnonzero(k["lm"][:n - m] >= 0), m, replace=False)
    for j, s in enumerate(src):
        t = n - m + j
        for name in ("keylines", "ldesc", "depth_line", "lines3d", "lm"):
            k[name][t] = k[name][s]
        k["keylines"]["start_x"][t] += np.float32(0.25)
        k["occupied"][t] = 0; k["occupied"][s] = 0


def new_lines_case(B=1, K=3, N=30, stride=None, seed=1, L=None, N2=None, bits=24, clutter=0.2, stereo=0.6, occupied=0.1, dup=2, shove=0.2, bad3d=0.25,
                   octave_off=0.3, pix=0.3, n_neigh=None, vary=True, seg=1.0, move0=0):
    """-> cam, cur (B key frames), neigh (B * K key frames), n_neigh [B].  N2: the neighbours' line count (default: at most the current key frame's)"""
    rng = np.random.default_rng(seed)
    S = stride or N
    L = L or 2 * N
    cam = NC.camera()
    mb = np.float32(np.float32(40.0) / cam["fx"])
    p = dict(bits=bits, clutter=clutter, stereo=stereo, occupied=occupied, octave_off=octave_off, pix=pix, bad3d=bad3d)
    cur_l, nb_l = [], []
    for b in range(B):
        mid = np.stack([rng.uniform(-2.5, 2.5, L), rng.uniform(-1.8, 1.8, L), rng.uniform(1.5, 7.0, L)], 1)
        half = rng.normal(size=(L, 3)) * np.array([0.35, 0.35, 0.5]) * seg
        P, Q = mid - half, mid + half
        desc_lm = rng.integers(0, 256, (L, 32)).astype(np.uint8)
        R1, C1 = NC._rot(rng, 4), rng.normal(size=3) * 0.05
        n1 = N - (int(rng.integers(0, 5)) if vary else 0)
        k1 = _observe(rng, cam, NC._pose(R1, C1), P, Q, np.arange(L), desc_lm, n1, S, p, 0.0)
        _duplicate(rng, k1, dup)
        cur_l.append(k1)
        for k in range(K):
            side = np.cross(R1[2], rng.normal(size=3)); side /= np.linalg.norm(side)
            mv = MOVES[(k + move0) % len(MOVES)]
            R2 = NC._rot(rng, 3) @ R1
            n2 = (N2 if N2 else n1) - (int(rng.integers(0, 6)) if vary else 0)
            nb_l.append(_observe(rng, cam, NC._pose(R2, C1 + side * mv[0] + R1[2] * mv[1]), P, Q, np.arange(L), desc_lm, n2, S, p, shove))

    def pack(lst):
        out = {name: np.stack([np.asarray(k[name]) for k in lst]) for name in ("keylines", "ldesc", "occupied", "depth_line", "lines3d", "Tcw")}
        out["n"] = np.array([k["n"] for k in lst], np.int32)
        out["Twc"] = np.stack([NC.set_pose_twc(k["Tcw"]).reshape(16) for k in lst])
        out["mb"] = np.full(len(lst), mb, np.float32)
        return out
    nn = np.full(B, K, np.int32) if n_neigh is None else np.asarray(n_neigh, np.int32)
    return cam, pack(cur_l), pack(nb_l), nn


# (name, arguments): the cases of tests/golden/new_lines_ref.npz, made by the real reference: no neighbour has more lines than its current key frame
CASES = [
    ("small", dict(B=3, K=3, N=32, stride=48, seed=611)),
    ("wide", dict(B=1, K=2, N=150, stride=160, seed=612, dup=6, move0=2)),
]
# restatement only: neighbours with more lines than the current key frame (idx2 >= n1 in the bStereo2 read counts as not stereo), more neighbours
HOST_CASES = [
    ("past_n1", dict(B=4, K=5, N=40, N2=70, stride=80, seed=621)),
    ("long_segments", dict(B=6, K=4, N=60, stride=64, seed=638, seg=3.0, octave_off=0.9, bad3d=0.0, shove=0.0, stereo=0.9)),   # the end points' scale tests disagree
]


def average_dir_case(seed=631, G=2, S=24, M=5):
    """map lines of G reference key frames, each observed by a subset of M key frames that holds the reference one (index 1) -> dict"""
    rng = np.random.default_rng(seed)
    cam = NC.camera()
    T = np.stack([np.stack([NC._pose(NC._rot(rng, 6), rng.normal(size=3) * 0.4) for _ in range(M)]) for _ in range(G)])      # [G, M, 4, 4]
    n = np.array([S, S - 5][:G] + [S] * max(0, G - 2), np.int32)
    mid = np.stack([rng.uniform(-2, 2, (G, S)), rng.uniform(-2, 2, (G, S)), rng.uniform(1.5, 7, (G, S))], 2)
    half = rng.normal(size=(G, S, 3)) * 0.4
    xw6 = np.concatenate([(mid - half).astype(np.float32), (mid + half).astype(np.float32)], 2).astype(np.float64)   # MapLine's Vector6d holds widened floats
    octave = rng.integers(0, 8, (G, S)).astype(np.int32)
    seen = rng.random((G, S, M)) < 0.5
    seen[:, :, 1] = True
    off = np.concatenate([[0], np.cumsum(seen.reshape(G * S, M).sum(1))]).astype(np.int32)
    Ow = np.stack([[NC.set_pose_twc(T[g, m])[:3, 3] for m in range(M)] for g in range(G)]).astype(np.float32)              # [G, M, 3]
    obs_ow = np.concatenate([Ow[g][seen[g, i]] for g in range(G) for i in range(S)]).astype(np.float32)
    return dict(cam=cam, T=T.astype(np.float32), n=n, xw6=xw6, octave=octave, seen=seen, obs_off=off, obs_ow=obs_ow, ref_Tcw=T[:, 1].reshape(G, 16).astype(np.float32))


# ---- the block files of the reference driver (tools/new_lines_golden): sequences of {int64 nbytes; bytes}
def kf_blocks(kf, e):
    n = int(kf["n"][e])
    return [np.ascontiguousarray(kf["keylines"][e, :n]), kf["ldesc"][e, :n], kf["occupied"][e, :n].astype(np.uint8), kf["depth_line"][e, :n].astype(np.float32),
            kf["lines3d"][e, :n].astype(np.float64), kf["Tcw"][e].astype(np.float32), np.array([kf["mb"][e]], np.float32)]


def create_blocks(cam, cur, neigh, nn, K, b, mode=0):
    blocks = [np.array([mode, nn[b]], np.int32), NC.cam_block(cam)] + kf_blocks(cur, b)
    for k in range(nn[b]):
        blocks += kf_blocks(neigh, b * K + k)
    return blocks


def average_dir_blocks(d, g):
    S = int(d["n"][g])
    return [np.array([2, d["T"].shape[1]], np.int32), NC.cam_block(d["cam"]), d["T"][g].astype(np.float32), d["xw6"][g, :S], d["octave"][g, :S].astype(np.int32),
            d["seen"][g, :S].astype(np.uint8)]


write_blocks, read_blocks = NC.write_blocks, NC.read_blocks
