"""Build guard (no GPU needed: hipcc cross-compiles): lsd_detect runs one wavefront per frame and shares its compute unit with the other one-wavefront-per-frame
kernels, so it must keep fitting four wavefronts per SIMD (512 / 4 = 128 VGPRs, nothing in scratch) and sixteen workgroups' dynamic LDS per CU (10 240 B each)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "lsd.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_lsd_detect_registers_and_scratch(tmp_path):
    out = tmp_path / "lsd.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    blocks = [b for b in meta.split("  - .agpr_count:") if re.search(r"\.name:\s+_ZN6planar3lsd10lsd_detectE", b)]
    assert len(blocks) == 1
    get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blocks[0]).group(1))
    print("lsd_detect: vgpr_count", get("vgpr_count"), "private_segment_fixed_size", get("private_segment_fixed_size"), "static LDS", get("group_segment_fixed_size"))
    assert get("private_segment_fixed_size") == 0
    assert get("vgpr_count") <= 128
    assert get("group_segment_fixed_size") == 0          # all of its LDS is the dynamic block sized below


def test_lsd_detect_dynamic_lds():
    """detect_smem as planar_lsd_create computes it, from the constants of lsd.hip."""
    text = open(SRC).read()
    m = re.search(r"o->detect_smem = ([^;]+);", text)
    assert m, "planar_lsd_create no longer sizes detect_smem in one expression"
    consts = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", text).group(1)) for k in ("RING", "USED_LDS_BITS")}
    expr = m.group(1).replace("lsd::", "").replace("/", "//")
    assert re.fullmatch(r"[\w\s+*/()]+", expr), expr
    smem = eval(expr, {"__builtins__": {}}, consts)
    print("lsd_detect: dynamic LDS", smem, "B")
    assert smem <= 10240
