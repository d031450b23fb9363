"""bench.py's command line, the parts that need no GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_bench_refuses_environment_switches():
    """No timing / variant switch reaches the timed region through the environment: bench.py exits non-zero when a PLANAR_* variable other than the developer-library
    override is set (round 4's PLANAR_TRACK_SKIP / PLANAR_PEAC_AHC / PLANAR_PEAC_WIDE no longer exist in the product either: planarslam_amd/ reads none of them)."""
    env = dict(os.environ, PLANAR_TRACK_SKIP="lsd")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "refusing to run" in (p.stderr + p.stdout)


def test_the_product_reads_no_timing_switch():
    import re
    pat = re.compile(r"getenv|os\.environ")
    hits = []
    for base, _, files in os.walk(os.path.join(ROOT, "planarslam_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".inc")):
                for n, line in enumerate(open(os.path.join(base, f), errors="replace"), 1):
                    if pat.search(line) and not re.search(r"PLANAR_HIP_LIB|RANK|WORLD_SIZE|MASTER_ADDR", line):
                        hits.append(f"{f}:{n}: {line.strip()}")
    assert not hits, hits


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    s = bench.dump_streams(2048)
    assert len(s) == bench.DUMP_STREAMS and np.array_equal(s, bench.dump_streams(2048)) and np.all(np.diff(s) > 0)
    a = bench.upto(np.ones((3, 4, 2), np.uint8), np.array([0, 2, 4]))
    assert a[:, :, 0].tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]]
    bench.dump_outputs(str(tmp_path), {"u8": np.arange(5, dtype=np.uint8), "i32": np.array([-7, 1 << 24], np.int32), "big": np.array([(1 << 24) + 1], np.int32),
                                       "f64": np.array([0.1]), "f32": np.array([0.1], np.float32)})
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert {k: v.dtype for k, v in got.items()} == {"u8": np.float32, "i32": np.float32, "big": np.float64, "f64": np.float64, "f32": np.float32}
    assert got["big"][0] == (1 << 24) + 1 and got["f64"][0] == 0.1 and got["i32"].tolist() == [-7, 1 << 24]
    p = subprocess.run([sys.executable, "-c", "import sys, numpy as np; sys.path.insert(0, %r); import bench; bench.dump_outputs(%r, {'x': np.zeros(1 << 25)})"
                        % (ROOT, str(tmp_path / "big"))], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "limit" in p.stderr and not os.path.exists(tmp_path / "big")
