"""CPU test: the KeyFrameDatabase adapter (include/planar_adapters.hpp, PLANAR_ADAPTERS_WITH_KFDB) compiles against stand-in key frames and links against
libplanar_hip.so; the program the GPU test runs (tests/adapter_shim/adapter_kfdb_main.cpp) builds here too.  No GPU call is made."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kfdb_adapter_compiles_and_links(tmp_path):
    from test_adapter_kfdb_gpu import build_command
    assert os.path.exists(os.path.join(ROOT, "planarslam_amd", "libplanar_hip.so")), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exe = str(tmp_path / "adapter_kfdb")
    subprocess.check_call(build_command(exe))
    assert subprocess.call([exe]) == 2          # no arguments: the usage exit, before anything touches a device
    header = open(os.path.join(ROOT, "include", "planar_adapters.hpp")).read()
    body = header[header.index("#ifdef PLANAR_ADAPTERS_WITH_KFDB"):header.index("#endif   // PLANAR_ADAPTERS_WITH_KFDB")]
    for signature in ("explicit KeyFrameDatabaseT(const VocabularyT&)", "void add(KeyFrameT* pKF)", "void erase(KeyFrameT* pKF)", "void clear()",
                      "std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore)", "std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F)"):
        assert signature in body, signature
