"""Build guard (no GPU needed: hipcc cross-compiles): normals_kernel and line3d_kernel are the last kernels of the plane and of the line stream and share their
compute units with the other streams' kernels, so neither may start to use scratch, nor need more registers or LDS per workgroup, nor fit fewer wavefronts per
SIMD than before their order-bound FP64 chains were spread over lanes.

The figures of the commit before (code-object notes of the same compile line):
    normals_kernel  86 VGPRs, 82 SGPRs, no scratch, no static LDS, 5 wavefronts per SIMD; 15 456 B of dynamic LDS at 640 x 480
    line3d_kernel  134 VGPRs, 68 SGPRs, 112 B of scratch, 3 136 B of static LDS, 3 wavefronts per SIMD
This commit: normals_kernel 63 / 78 / 0 / 0 / 8 and 15 456 B; line3d_kernel 128 / 68 / 0 / 3 136 / 4."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "planarslam_amd", "csrc")

# kernel -> (source, mangled-name pattern, VGPRs, SGPRs, static LDS, wavefronts per SIMD) of the commit before
BEFORE = {
    "normals_kernel": ("normals.hip", r"_ZN6planar7normals14normals_kernelE", 86, 82, 0, 5),
    "line3d_kernel": ("line3d.hip", r"_ZN6planar6line3d13line3d_kernelE", 134, 68, 3136, 3),
}


def waves_per_simd(vgprs):
    """gfx950: 512 registers per SIMD lane, handed out in blocks of 8, at most 8 wavefronts"""
    return min(8, 512 // (-(-vgprs // 8) * 8))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("kernel", list(BEFORE))
def test_registers_lds_scratch_and_occupancy(tmp_path, kernel):
    src, pattern, vgprs, sgprs, lds, waves = BEFORE[kernel]
    assert waves_per_simd(vgprs) == waves
    out = tmp_path / (kernel + ".s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only",
                           os.path.join(CSRC, src), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    blocks = [b for b in meta.split("  - .agpr_count:") if re.search(r"\.name:\s+" + pattern, b)]
    assert len(blocks) == 1
    get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blocks[0]).group(1))
    agprs = int(re.match(r"\s*(\d+)", blocks[0]).group(1))
    got = dict(vgpr=get("vgpr_count"), agpr=agprs, sgpr=get("sgpr_count"), scratch=get("private_segment_fixed_size"), lds=get("group_segment_fixed_size"))
    print(kernel, got, "wavefronts per SIMD", waves_per_simd(got["vgpr"] + got["agpr"]))
    assert got["scratch"] == 0 and get("vgpr_spill_count") == 0          # (scalar registers parked in lanes of a vector register are not memory)
    assert got["vgpr"] + got["agpr"] <= vgprs
    assert got["sgpr"] <= sgprs
    assert got["lds"] <= lds
    assert waves_per_simd(got["vgpr"] + got["agpr"]) >= waves


def test_normals_dynamic_lds():
    """what planar_normals_create asks for, from the constants of normals.hip: no more than the row-by-row kernel's max(2 gw + 2 floats, iw x 6 doubles + gw x 6 floats)"""
    text = open(os.path.join(CSRC, "normals.hip")).read()
    rb = int(re.search(r"constexpr int RB = (\d+);", text).group(1))
    m = re.search(r"p->smem = std::max\(([^;]+)\);", text)
    assert m, "planar_normals_create no longer sizes its LDS in one expression"
    expr = m.group(1).replace("(size_t)", "").replace("normals::RB", str(rb)).replace("G.", "")
    assert re.fullmatch(r"[\w\s+*(),]+", expr), expr
    for w in (96, 640, 1280, 2050, 4096):
        gw = -(-w // 3)
        now = max(*eval("(" + expr + ")", {"__builtins__": {}}, {"gw": gw, "iw": gw + 1}))
        before = max((2 * gw + 2) * 4, (gw + 1) * 6 * 8 + gw * 6 * 4)
        print("normals_kernel: dynamic LDS at width", w, now, "B, before", before, "B")
        assert now <= before
    assert max(*eval("(" + expr + ")", {"__builtins__": {}}, {"gw": 214, "iw": 215})) == 15456
