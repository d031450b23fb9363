#!/usr/bin/env python3
"""Generate tests/golden/orb_*.npz: inputs + outputs of the REAL reference ORBextractor
(oracle/_ref/ref_orb = the reference's src/ORBextractor.cc compiled against oracle/shim).

    tools/gen_golden_orb.py                 every fixture
    tools/gen_golden_orb.py wide960 noise   the named ones only (the others stay as they are)

Runs only where oracle/_ref is built; R1 and OFF1 also need the reference's example images
(the REF variable of oracle/Makefile, same default).  The committed fixtures
travel to the GPU box, where the reference does not exist.
"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol
import orb_cases as oc
from planarslam_amd.synth import gray_image

DEFAULT = dict(nfeatures=1000, scale=1.2, nlevels=8, ini=20, mn=7)


def natural(name):
    from PIL import Image
    a = np.asarray(Image.open(os.path.join(os.environ.get("REF", "/root/reference"), "Examples", f"{name}.png")).convert("L"))
    return a[40:520, 60:700].copy()


# name -> (image builder, parameters); the builders run only for the names asked for
CASES = {
    "R1": (lambda: natural("R1"), DEFAULT),
    "OFF1": (lambda: natural("OFF1"), DEFAULT),
    "synth1234": (lambda: gray_image(1234), DEFAULT),
    "noise": (lambda: np.random.default_rng(5).integers(0, 256, (240, 320)).astype(np.uint8), dict(nfeatures=500, scale=1.2, nlevels=4, ini=20, mn=7)),
    "odd517": (lambda: gray_image(10, 517, 389), dict(nfeatures=700, scale=1.3, nlevels=5, ini=25, mn=9)),
}
# cases of tests/orb_cases.py: more than one initial octree node, a 32-bit path code, fewer features than initial nodes
for key, case in oc.GOLDEN.items():
    CASES[key] = (oc.BY_NAME[case].image, oc.BY_NAME[case].params)


def main(names):
    unknown = [n for n in names if n not in CASES]
    if unknown:
        sys.exit(f"unknown fixture(s) {unknown}; known: {list(CASES)}")
    out = os.path.join(ROOT, "tests", "golden")
    for name in names or list(CASES):
        build, p = CASES[name]
        img = build()
        kps, desc, pyr = ol.run_ref_orb(img, **p)
        np.savez_compressed(os.path.join(out, f"orb_{name}.npz"), image=img, kps=kps, desc=desc,
                            params=np.array([p["nfeatures"], p["scale"], p["nlevels"], p["ini"], p["mn"]], np.float64),
                            level_shapes=np.array([q.shape for q in pyr], np.int32),
                            level_sums=np.array([int(q.astype(np.int64).sum()) for q in pyr], np.int64),
                            last_level=pyr[-1])
        print(name, img.shape, len(kps))


if __name__ == "__main__":
    main(sys.argv[1:])
