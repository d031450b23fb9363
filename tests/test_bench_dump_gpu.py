"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, written as .npy files after the timed region.  Two runs with the same
arguments write the same arrays; one more timed step changes them (the last step is a different frame of every stream); a plain run (no --full) writes
what a --full run writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("--batch", "32", "--canvases", "8", "--warmup", "1")
SMALL = PLAIN + ("--full", "--cpu-seconds", "0", "--latency-reps", "0", "--pcie-steps", "0", "--sub-steps", "0")


def _bench(out, *flags, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(out), *flags], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    names = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in names}


def test_full_workload_dumps_the_same_outputs_for_the_same_arguments(tmp_path):
    a, b, c, p = tmp_path / "a", tmp_path / "b", tmp_path / "c", tmp_path / "p"
    da = _bench(a, "--steps", "2", *SMALL)
    _bench(b, "--steps", "2", *SMALL)
    dc = _bench(c, "--steps", "3", *SMALL)
    assert da["steps"] == 2 and dc["steps"] == 3 and da["parity_sample"]["ok"]
    A, B_, C = _load(a), _load(b), _load(c)
    assert sum(x.nbytes for x in A.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in A.values())
    kp = A["orb_keypoints"][0, :int(A["orb_count"][int(A["sample_streams"][0])])]
    assert (kp[:, 5] >= 0).all() and (kp[:, 5] < 8).all() and (kp[:, 6] == -1).all(), "octave / class_id are the key points' integers"
    assert {"orb_keypoints", "orb_descriptors", "line_keylines", "plane_labels", "planes", "plane_points", "pose_opt_Tcw", "Tcw"} <= set(A)
    assert A["Tcw"].shape == (32, 16) and A["orb_count"].shape == (32,) and A["orb_count"].min() > 100
    s = A["sample_streams"].astype(int)
    assert len(s) == 16 and A["orb_keypoints"].shape[0] == 16 and A["plane_labels"].shape == (16, 480, 640)
    assert A.keys() == B_.keys() and all(np.array_equal(A[k], B_[k]) for k in A), [k for k in A if not np.array_equal(A[k], B_[k])]
    assert not np.array_equal(A["orb_keypoints"], C["orb_keypoints"]), "--steps 3 dumped the same last step as --steps 2"
    # without --full: the same timed steps and outputs, none of the extra legs
    dp = _bench(p, "--steps", "2", *PLAIN)
    P = _load(p)
    assert A.keys() == P.keys() and all(np.array_equal(A[k], P[k]) for k in A), [k for k in A if not np.array_equal(A[k], P[k])]
    assert dp["steps"] == 2 and dp["value"] > 0 and dp["ms_per_step"] > 0
    assert all(dp[k] is None for k in ("parity_sample", "roofline", "cpu_baseline", "latency_b1_ms", "sub_benchmarks", "value_pcie_inclusive"))


def test_pose_workload_dumps_its_batch(tmp_path):
    d = _bench(tmp_path, "--workload", "pose", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0")
    assert d["steps"] == 2
    A = _load(tmp_path)
    assert A["Tcw_out"].shape == (256, 16) and A["n_inliers"].min() > 0 and np.isfinite(A["Tcw_out"]).all()
