"""CPU test: the shared gathers of include/planar_adapters.hpp (planar_adapter::ViewGather, PointGather), part by part, in a stand-alone program
(tests/adapter_shim/adapter_gather_main.cpp) that builds stand-in Frame / KeyFrame / MapPoint objects from known arrays and compares every field of the views with
them: n = 0 and n = 3, mvuRight empty and filled, blocked on and off, the pose from mTcw / GetPose() / [R | t], the camera from members and from mK, 20 and 5 scale
factors with and without the 1.f pre-fill, a point list with a NULL, a bad and a good point with and without the exclusion and the optional arrays, and copies of both
gathers.  The program makes no device call and links without libplanar_hip.so.  It is built twice, plain and with the address and undefined-behaviour sanitizers,
and each build runs as an ordinary child process."""
import subprocess

import pytest

from adapter_build import build_command, shim_source


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")], ids=["plain", "sanitized"])
def test_gathers_equal_the_arrays_they_were_built_from(tmp_path, flags):
    exe = str(tmp_path / "adapter_gather")
    subprocess.check_call(build_command(exe, [shim_source("adapter_gather_main.cpp")], library=False, flags=flags))
    assert subprocess.call([exe]) == 0
