"""CPU: what the frames of tests/lsd_path_cases.py are for, confirmed with the oracle alone (oracle/lsd_oracle.cpp) - every frame yields lines, the `ring` frames hold
a kept region of more than RING points, the `used_tail` frame more than USED_LDS_BITS defined pixels.  (Whether a frame takes refine()'s re-grow is a count only the
kernel keeps: tests/test_lsd_detect_paths_gpu.py asserts it on the device.)"""
import numpy as np
import pytest

import lsd_path_cases as LC
import oracle_lib as O


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_frame_serves_its_paths(name):
    make, paths = LC.CASES[name]
    img = make()
    ref = O.lsd_detect(img, tie_order=0, want_stages=True)
    kl, desc, eq, _, n_detected = O.extract_line_segment(img, tie_order=0)
    defined = int((ref["angles"] != -1024.0).sum())
    longest = LC.min_region_points(ref["xy"], ref["wpn"][:, 0]).max(initial=0)
    print(f"{name}: {img.shape[1]}x{img.shape[0]}, {defined} defined pixels, {len(ref['xy'])} raw segments, {len(kl)} key lines, largest kept region >= {longest:.0f} points")
    assert len(kl) >= 1 and n_detected == len(ref["xy"]) >= 1
    if "ring" in paths or "many_accepts" in paths:
        assert longest > LC.RING
    if "used_tail" in paths:
        assert defined > LC.USED_LDS_BITS
    if name.startswith("hd"):
        assert img.shape == (720, 1280)
    if name.startswith("offgrid"):
        assert img.shape[0] % 8 and img.shape[1] % 8
