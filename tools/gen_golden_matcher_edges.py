"""Generate tests/golden/matcher_edges_ref.npz: the outputs of the REAL reference matchers and Frame::isInFrustum on the cases of
tests/matcher_edge_cases.py (distorted views and gate cases).  oracle/_ref/ref_match and oracle/_ref/ref_frame run them through the wrappers of
tests/oracle_lib.py; the key-frame overload of SearchByProjection goes through the driver of tools/gen_golden_kf_proj.py, built by the same recipe.  Inputs are
regenerated from seeds by the cases module; only outputs are stored, as one int32 vector (floats by their bits) with an offset per call.
    python tools/gen_golden_matcher_edges.py [/path/to/reference]"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_kf_proj as GK  # noqa: E402
import matcher_edge_cases as M  # noqa: E402
import oracle_lib as O  # noqa: E402


def run_ref(c, exe, tmp):
    """the reference's outputs of one call, shaped as matcher_edge_cases.run_oracle shapes the oracle's"""
    e = c["entry"]
    if e in ("frame", "map", "kf", "bow"):
        fr = c["f"]["node"] if e == "bow" else c["frame" if e == "map" else "cur"]["keys_un"]
        B, S = fr.shape
        m = np.full((B, S), -1, np.int32); n = np.zeros(B, np.int32)
        for b in range(B):
            if e == "frame":
                mb, nb = O.ref_search_by_projection_frame(c["cur"], c["last"], b, c["th"], mono=c["mono"], check_orientation=c["ori"])
            elif e == "map":
                mb, nb = O.ref_search_by_projection_map(c["frame"], c["probes"], b, c["th"], c["ratio"])
            elif e == "kf":
                mb, nb = GK.run_pair(exe, tmp, c["cur"], c["kf"], b, c["th"], c["orb"], c["ori"], lsf=M.kf_lsf(c))
            else:
                mb, nb = O.ref_search_by_bow(c["kf"], c["f"], b, c["ratio"], check_orientation=c["ori"])
            m[b, :len(mb)] = mb; n[b] = nb
        return dict(match=m, n=n)
    if e == "lsd_proj":
        safe = M.ref_safe_proj_lines(c)
        B, S = c["lines"]["keylines"].shape
        m = np.full((B, S), -1, np.int32); n = np.zeros(B, np.int32)
        for b in range(B):
            mb, n[b] = O.ref_lsd_search_by_projection(c["lines"], safe["ml"], b, c["sf"], c["th"], c["ratio"])
            m[b, :len(mb)] = mb
        return dict(match=m, n=n)
    if e in ("fuse", "lsd_fuse"):
        safe = M.ref_safe_lines(c) if e == "lsd_fuse" else c
        pts = safe["mp" if e == "fuse" else "ml"]
        B, S = pts["usable"].shape
        idx = np.full((B, S), -1, np.int32); nf = np.zeros(B, np.int32)
        for b in range(B):
            if e == "fuse":
                r, k = O.ref_fuse(c["kf"], pts, b, c["th"], c["lsf"], c["nlev"], inv_level_sigma2=c.get("inv_sigma2"))
            else:
                r, k = O.ref_lsd_fuse(c["kf"], c["lines"], pts, b, c["th"], c["lsf"], c["nlev"])
            idx[b, :len(r)] = r; nf[b] = k
        return dict(fuse_idx=idx, n_fused=nf)
    pts = c["mp" if e == "frustum_points" else "ml"]
    B, S = pts["valid"].shape
    out = dict(in_view=np.zeros((B, S), np.uint8), level=np.zeros((B, S), np.int32), view_cos=np.zeros((B, S), np.float32))
    if e == "frustum_points":
        out.update(proj_x=np.zeros((B, S), np.float32), proj_y=np.zeros((B, S), np.float32), proj_xr=np.zeros((B, S), np.float32))
    else:
        out["proj"] = np.zeros((B, S, 4), np.float32)
    for b in range(B):
        if e == "frustum_points":
            i, rec = O.run_ref_frustum_points(c["frame"], pts, b, c["lsf"], c["nlev"], limit=c["limit"])
            out["in_view"][b, i] = rec["in_view"]
            assert np.array_equal(rec["ret"], rec["in_view"])
            for k, r in (("proj_x", "px"), ("proj_y", "py"), ("proj_xr", "pxr"), ("level", "level"), ("view_cos", "vc")):
                out[k][b, i] = rec[r]
        else:
            i, rec = O.run_ref_frustum_lines(c["frame"], pts, b, c["lsf"], limit=c["limit"])
            out["in_view"][b, i] = rec["ret"]; out["proj"][b, i] = rec["p"]; out["level"][b, i] = rec["level"]; out["view_cos"][b, i] = rec["vc"]
    return M.mask_frustum(out, M.OUT[e])


def main():
    names, off, data = [], [0], []
    with tempfile.TemporaryDirectory() as tmp:
        exe = GK.build(tmp)
        for name, c in M.all_calls():
            v = M.flat(c["entry"], run_ref(c, exe, tmp))
            names.append(name); data.append(v); off.append(off[-1] + len(v))
    dst = os.path.join(ROOT, "tests", "golden", "matcher_edges_ref.npz")
    np.savez_compressed(dst, names=np.array(names), off=np.array(off, np.int64), data=np.concatenate(data).astype(np.int32))
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(names), "calls")


if __name__ == "__main__":
    main()
