"""Inputs of tests/test_spec_resolve_gpu.py: SearchByProjection(Cur, Last) and SearchByProjection(Frame, MapPoints) problems built to drive the speculating resolver of
planarslam_amd/csrc/guided.hip through its rounds, its fallback and its chunk cuts, and the numpy measure of how much the probes of a 256-probe chunk share."""
import numpy as np

from planarslam_amd import synth

SPEC_MAX_LIST = 64     # planarslam_amd/csrc/match_chunk.h
CAND_CAP = 8192
CHUNK = 256


def map_windows(fr, pr, b, th):
    """per probe of frame b, in order: the key-point indices of its window (the square window, the level gate [level - 1, level] and the stereo gate of
    ORBmatcher::SearchByProjection(F, vpMapPoints, th), src/ORBmatcher.cc:46-130, in float32), [] for a probe that is not in view"""
    n, k = int(fr["n"][b]), fr["keys_un"][b]
    x, y, octv, uR = k["x"][:n], k["y"][:n], k["octave"][:n].astype(int), fr["u_right"][b, :n]
    out = []
    for j in range(int(pr["n"][b])):
        if not pr["in_view"][b, j]:
            out.append(np.zeros(0, int)); continue
        lvl = int(pr["level"][b, j])
        r = np.float32(2.5 if float(pr["view_cos"][b, j]) > 0.998 else 4.0)
        if th != 1.0:
            r = np.float32(r * np.float32(th))
        r = np.float32(r * fr["scale_factors"][lvl])
        u, v, ur = pr["proj_x"][b, j], pr["proj_y"][b, j], pr["proj_xr"][b, j]
        ok = (np.abs(x - u) < r) & (np.abs(y - v) < r) & (octv >= lvl - 1) & (octv <= lvl)
        ok &= ~((uR > 0) & (np.abs(ur - uR) > r))
        out.append(np.nonzero(ok)[0])
    return out


def frame_windows(cur, last, b, th):
    """the same for SearchByProjection(Cur, Last, th) (src/ORBmatcher.cc:1396-1535) with a still camera: the square window around the projection (float64: a
    statistic of the inputs, not a bit-exact list) and the level gate [octave - 1, octave + 1]"""
    n, k = int(cur["n"][b]), cur["keys_un"][b]
    x, y, octv = k["x"][:n].astype(float), k["y"][:n].astype(float), k["octave"][:n].astype(int)
    T = cur["Tcw"][b].reshape(4, 4).astype(float)
    out = []
    for j in range(int(last["n"][b])):
        X = T[:3, :3] @ last["xw"][b, j].astype(float) + T[:3, 3]
        if not last["usable"][b, j] or X[2] <= 0:
            out.append(np.zeros(0, int)); continue
        u, v = cur["fx"] * X[0] / X[2] + cur["cx"], cur["fy"] * X[1] / X[2] + cur["cy"]
        o = int(last["octave"][b, j])
        r = th * float(cur["scale_factors"][o])
        out.append(np.nonzero((np.abs(x - u) < r) & (np.abs(y - v) < r) & (octv >= o - 1) & (octv <= o + 1))[0])
    return out


def shared_share(windows):
    """the share of probes whose window holds a key point that also lies in the window of an earlier probe of the same 256-probe chunk"""
    hit = 0
    for c in range(0, len(windows), CHUNK):
        seen = set()
        for w in windows[c:c + CHUNK]:
            hit += any(int(i) in seen for i in w)
            seen.update(int(i) for i in w)
    return hit / max(1, len(windows))


def crowded(N=300, crowd=0.7, dup=0.9, seed=301, all_observed=False, B=3):
    """a crowded current frame and a last frame whose map points mostly compete for the same key points"""
    fr = synth.guided_frame(B=B, N=N, seed=seed, crowd=crowd)
    cur, last = synth.guided_last_frame(fr, seed=seed + 1, dup=dup)
    if all_observed:
        last["mp_observed"][:] = 1
    return cur, last


def crowded_map(N=300, crowd=0.7, n_probes=700, seed=311, all_observed=False, equal_levels=False, B=3):
    """... for the map search.  The crowded key points carry noisy copies (up to 40 bits) of four descriptors, so a probe's second best is often close enough for
    the ratio test to reject it: the match counts differ between nn_ratio 0.6 and 0.8"""
    fr = synth.guided_frame(B=B, N=N, seed=seed, crowd=crowd)
    rng = np.random.default_rng(seed + 2)
    proto = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    for b in range(B):
        nc = int(crowd * int(fr["n"][b]))
        fr["desc"][b, :nc] = synth._flip_bits(rng, proto[rng.integers(0, 4, nc)], 40)
    if equal_levels:
        fr["keys_un"]["octave"][:] = 2
    fr, pr = synth.guided_map_probes(fr, seed=seed + 1, n_probes=n_probes)
    if equal_levels:
        pr["level"][:] = 2
    if all_observed:
        pr["observed"][:] = 1
    return fr, pr


def _bare_frame(xy, octave=1, seed=321, same_desc=False):
    """one frame (B = 1) with key points at xy [N, 2], one octave, no stereo coordinate, nothing blocked"""
    N = len(xy)
    fr = synth.guided_frame(B=1, N=N, seed=seed, crowd=0.0)
    fr["keys_un"]["x"][0, :N] = xy[:, 0]; fr["keys_un"]["y"][0, :N] = xy[:, 1]
    fr["keys_un"]["octave"][0, :N] = octave
    fr["u_right"][:] = -1
    if same_desc:
        fr["desc"][0, :] = fr["desc"][0, 0]
    fr["blocked"] = np.zeros(fr["keys_un"].shape, np.uint8)
    return fr


def _probes_at(fr, at, level=1, seed=331, observed=None, exact_desc=False, bits=20):
    """map probes of frame 0 projecting exactly onto the key points at[j]; descriptors are noisy copies of theirs (exact ones with exact_desc)"""
    rng = np.random.default_rng(seed)
    P = len(at)
    k = fr["keys_un"][0, at]
    desc = fr["desc"][0, at] if exact_desc else synth._flip_bits(rng, fr["desc"][0, at], bits)
    return dict(n=np.array([P], np.int32), in_view=np.ones((1, P), np.uint8), proj_x=k["x"][None].astype(np.float32), proj_y=k["y"][None].astype(np.float32),
                proj_xr=np.full((1, P), -1, np.float32), level=np.full((1, P), level, np.int32), view_cos=np.full((1, P), 0.9, np.float32),
                desc=np.ascontiguousarray(desc[None]), observed=(rng.random((1, P)) < 0.5).astype(np.uint8) if observed is None else np.full((1, P), observed, np.uint8))


def one_shared_candidate(P=300, observed=None):
    """every probe's window holds key point 0 and nothing else (th = 1: r = 4 * 1.2 px; the other key points lie 100 px and more away)"""
    xy = np.array([[320.0, 240.0]] + [[20.0 + 9 * i, 30.0] for i in range(40)])
    fr = _bare_frame(xy)
    return fr, _probes_at(fr, np.zeros(P, int), observed=observed)


def no_shared_candidate():
    """key points on a 40 px lattice, one probe per key point, in a shuffled order: every window (r = 4.8 px) holds its own key point alone"""
    gx, gy = np.meshgrid(np.arange(20, 620, 40.0), np.arange(20, 460, 40.0))
    xy = np.stack([gx.ravel(), gy.ravel()], 1)
    fr = _bare_frame(xy, seed=322)
    return fr, _probes_at(fr, np.random.default_rng(5).permutation(len(xy)), seed=332)


def cluster(n_in, P=200, spread=3.0, same_desc=False, observed=None, extra=0):
    """n_in key points within `spread` px of (320, 240) and `extra` far ones; every probe projects onto one of the n_in, so every list holds exactly those n_in
    (r = 4.8 px at th = 1 would not cover them: the cases run at th = 3, r = 14.4 px)"""
    rng = np.random.default_rng(340 + n_in)
    xy = np.concatenate([np.array([320.0, 240.0]) + rng.uniform(-spread, spread, (n_in, 2)), np.stack([np.linspace(10, 630, extra), np.full(extra, 20.0)], 1)])
    fr = _bare_frame(xy, seed=341 + n_in, same_desc=same_desc)
    return fr, _probes_at(fr, rng.integers(0, n_in, P), seed=342 + n_in, observed=observed, exact_desc=same_desc)
