"""CPU test: the key-frame adapters (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_KEYFRAME) compile against stand-in classes and link against
libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_keyframe_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keyframe_adapters_compile_and_link(tmp_path):
    from test_adapter_keyframe_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_keyframe")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_KEYFRAME"):header.index("#endif   // PLANAR_ADAPTERS_WITH_KEYFRAME")]
    for text in ("inline bool Tracking::NeedNewKeyFrame()", "inline void Tracking::CreateNewKeyFrame()", "on_lane(planar_adapter::TRACKING, \"planar_need_new_key_frame\"",
                 "on_lane(planar_adapter::TRACKING, \"planar_create_new_key_frame\"", "mpLocalMapper->InterruptBA()", "created_pt[c]", "new MapPoint(x3D, pKF, mpMap)",
                 "pNewMP->AddObservation(pKF, i)", "mpMap->AddMapPoint(pNewMP)", "created_ml[c]", "new MapLine(line3D, pKF, mpMap)", "new MapPlane(p3D, pKF, mpMap)",
                 "mpLocalMapper->InsertKeyFrame(pKF)", "mnLastKeyFrameId = mCurrentFrame.mnId"):
        assert text in body, text
