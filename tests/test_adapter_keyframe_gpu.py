"""The key-frame adapters, executed: Tracking::NeedNewKeyFrame and Tracking::CreateNewKeyFrame (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_KEYFRAME) compiled
ON THE GPU BOX into tests/adapter_shim/adapter_keyframe_main.cpp against stand-in classes and run by the fixture generator's driver on cases the real reference
processed (tests/golden/keyframe_ref.npz).  What the program writes - the decision, InterruptBA, the cleaned matches; the frame's and the new key frame's matches,
the created points and lines in Map::AddMapPoint order with their key-point index and observation count - must equal the fixture's record, every integer."""
import subprocess

import numpy as np
import pytest

import adapter_build as AB
import keyframe_cases as KC
import keyframe_check as CK

pytestmark = pytest.mark.gpu
NEED = ["need_none", "need_c1a_alone", "need_c1b_false_rest_true", "need_c1c_false_rest_true", "need_nkfs_1", "need_nkfs_2", "need_inliers_by_lines_and_planes", "need_ratio_3_10",
        "need_ratio_299_1000", "need_ref_4x_plus_1", "need_new_plane_busy", "need_busy_queue_3", "need_only_tracking", "need_after_reloc", "need_id_wraps",
        "need_ghosts_in_map_ratio", "need_shared_map"]
CREATE = ["walk_close_0", "walk_far_102", "walk_c_101", "walk_ties", "walk_at_threshold", "sort_65", "sort_2048", "rule", "lines_52", "create_two_maps"]


def build_command(out):
    return AB.build_command(out, [AB.shim_source("adapter_keyframe_main.cpp")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapter_keyframe") / "adapter_keyframe")
    subprocess.check_call(build_command(out))
    return out


@pytest.mark.parametrize("name", NEED + CREATE)
def test_adapter_equals_the_reference(exe, tmp_path, name):
    case = KC.make(name)
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    KC.stream(case).tofile(pin)
    subprocess.run([exe, pin, pout], check=True, timeout=120, stdout=subprocess.DEVNULL)
    got, want = KC.parse_ref(case, np.fromfile(pout, np.int32)), KC.parse_ref(case, CK.ref(name))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in w:
            assert np.array_equal(g[k], w[k]), (name, k)
