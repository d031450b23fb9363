"""GPU parity: HIP pose-only LM (planar_pose_opt) vs the CPU oracle of Optimizer::PoseOptimization /
TranslationOptimization on seeded synthetic frames.  Tolerance (BASELINE.json north_star): 1e-5 on the
SE3 pose; outlier flags and the returned inlier count must be identical."""
import numpy as np
import pytest

import oracle_lib as ol
from planarslam_amd.synth import TUM3, pose_batch

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-5


def _compare(batch, mode, rounds=4, its=10):
    from planarslam_amd import Optimizer
    opt = Optimizer(TUM3)
    got = (opt.PoseOptimization if mode == 0 else opt.TranslationOptimization)(batch, rounds, its)
    want = ol.pose_optimize(batch, TUM3, mode, rounds, its)
    assert np.abs(got["Tcw"] - want["Tcw"]).max() <= POSE_TOL
    assert np.array_equal(got["n_inliers"], want["n_inliers"])
    assert np.array_equal(got["pt_outlier"], want["pt_outlier"])
    assert np.array_equal(got["ln_outlier"], want["ln_outlier"])
    assert np.array_equal(got["pl_outlier"], want["pl_outlier"])
    # LM iteration counts are diagnostic: a stop test sitting on a knife edge ((iniChi-chi)*1e3 < iniChi) may flip
    # with the reduction order, but then the pose has already converged (checked above).
    assert np.abs(got["lm_iters"] - want["lm_iters"]).max() <= 1
    return got, want


@pytest.mark.parametrize("mode", [0, 1])
def test_pose_c4_shape(mode):
    # BASELINE config 4 shape: 1000 points + 75 lines (150 endpoint edges) + 12 plane edges
    _compare(pose_batch(B=8, seed=7), mode)


def test_pose_recovers_ground_truth_without_noise_outliers():
    b = pose_batch(B=4, seed=100, outlier_frac=0.0)
    got, _ = _compare(b, 0)
    for i in range(4):
        T = got["Tcw"][i].reshape(4, 4)
        assert np.abs(T[:3, :3] - b["T_gt"][i][:3, :3]).max() < 5e-3
        assert np.abs(T[:3, 3] - b["T_gt"][i][:3, 3]).max() < 5e-3


@pytest.mark.parametrize("mode", [0, 1])
def test_pose_ragged_and_padded(mode):
    # different feature counts per frame inside padded strides; some frames without lines / planes
    b = pose_batch(B=6, n_points=300, n_lines=20, n_planes=3, seed=31, max_points=512, max_lines=40, max_planes=8)
    b["n_points"][:] = [300, 120, 7, 300, 64, 299]
    b["n_lines"][:] = [20, 0, 3, 20, 1, 19]
    b["n_planes"][:] = [3, 0, 1, 2, 3, 0]
    _compare(b, mode)


def test_pose_single_round_bench_shape():
    _compare(pose_batch(B=4, seed=55), 0, rounds=1, its=10)


def test_pose_too_few_correspondences_returns_zero():
    b = pose_batch(B=2, n_points=10, n_lines=0, n_planes=0, seed=3)
    b["pt_valid"][:] = 0
    b["pt_valid"][:, :2] = 1
    got, want = _compare(b, 0)
    assert (got["n_inliers"] == 0).all()
    assert np.array_equal(got["Tcw"], b["Tcw"])


def test_pose_only_points():
    _compare(pose_batch(B=3, n_lines=0, n_planes=0, seed=9, max_lines=4, max_planes=2), 0)


# ---- against the REAL reference (tests/golden/opt_ref.npz = outputs of src/Optimizer.cc + vendored g2o built as oracle/_ref/ref_opt) ----
import os

import opt_cases as cases
from test_oracle_opt_ref import golden_pose


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "opt_ref.npz"))


@pytest.mark.parametrize("name", list(cases.POSE_CASES))
def test_pose_hip_equals_reference_fixture(golden, name):
    """HIP PoseOptimization / TranslationOptimization vs what the reference's own functions returned on the same frames:
    1e-5 on the pose, identical outlier flags and return values.  c4_b256 is BASELINE config 4 at its batch size."""
    from planarslam_amd import Optimizer
    build, modes = cases.POSE_CASES[name]
    b = build()
    opt = Optimizer(TUM3)
    for mode in modes:
        got = (opt.PoseOptimization if mode == 0 else opt.TranslationOptimization)(b, 4, 10)
        want = golden_pose(golden, name, mode, b)
        assert np.abs(got["Tcw"] - want["Tcw"]).max() <= POSE_TOL
        assert np.array_equal(got["n_inliers"], want["n_inliers"])
        for k in ("pt_outlier", "ln_outlier", "pl_outlier"):
            assert np.array_equal(got[k], want[k]), k


# ---- regimes that the cases above never reach (opt_cases.POSE_REGIME_CASES, tests/golden/opt_pose_regimes.npz), and the entry points' contract ----
import ctypes as C

from test_oracle_opt_ref import POSE_REGIME_RUNS, pose_regime_run

EINVAL = -1
FILL = 0xA5
_OUT = ("Tcw", "pt_outlier", "ln_outlier", "pl_outlier", "n_inliers", "lm_iters")


@pytest.fixture(scope="module")
def pose_regimes(golden_dir):
    return np.load(os.path.join(golden_dir, "opt_pose_regimes.npz"))


def _outputs(batch, fill):
    B = len(batch["n_points"])
    MP, ML, MM = batch["pt_valid"].shape[1], batch["ln_valid"].shape[1], batch["pl_valid"].shape[1]
    return dict(Tcw=np.zeros((B, 16), np.float32), pt_outlier=np.full((B, MP), fill, np.uint8), ln_outlier=np.full((B, ML), fill, np.uint8),
                pl_outlier=np.full((B, MM, 3), fill, np.uint8), n_inliers=np.full(B, -77, np.int32), lm_iters=np.full(B, -77, np.int32))


def _pose_batch_struct(batch, out, addr, want_lm_iters=True):
    from planarslam_amd._lib import PoseBatch
    from planarslam_amd.optimizer import _IN
    pb = PoseBatch()
    pb.B, pb.max_points, pb.max_lines, pb.max_planes = len(batch["n_points"]), batch["pt_valid"].shape[1], batch["ln_valid"].shape[1], batch["pl_valid"].shape[1]
    for k in _IN:
        setattr(pb, k, addr(batch[k]))
    pb.Tcw_in = addr(batch["Tcw"])
    pb.Tcw_out, pb.pt_outlier, pb.ln_outlier, pb.pl_outlier, pb.n_inliers = (addr(out[k]) for k in _OUT[:5])
    pb.lm_iters = addr(out["lm_iters"]) if want_lm_iters else None
    return pb


def run_host(batch, params, mode, rounds=4, its=10, fill=0, want_lm_iters=True, patch=None):
    """planar_pose_opt on a PoseBatch built here: the output arrays start filled with `fill`; `patch(pb)` may bend the struct.  -> (return code, outputs)"""
    from planarslam_amd import Optimizer
    opt = Optimizer(params)
    batch = {k: np.ascontiguousarray(v) for k, v in batch.items()}
    out = _outputs(batch, fill)
    pb = _pose_batch_struct(batch, out, lambda a: a.ctypes.data, want_lm_iters)
    if patch:
        patch(pb)
    rc = opt.L.planar_pose_opt(opt.ctx.h, C.byref(pb), C.byref(opt.params), mode, rounds, its)
    return rc, out


def _same_as_oracle(got, want):
    assert np.abs(got["Tcw"] - want["Tcw"]).max() <= POSE_TOL
    for k in ("n_inliers", "pt_outlier", "ln_outlier", "pl_outlier"):
        assert np.array_equal(got[k], want[k]), k
    assert np.abs(got["lm_iters"] - want["lm_iters"]).max() <= 1


@pytest.mark.parametrize("name,mode", POSE_REGIME_RUNS)
def test_pose_hip_equals_regime_fixture(pose_regimes, name, mode):
    """HIP vs what the reference's own functions returned in each regime: 1e-5 on the pose, identical flags and return values; the LM iteration count
    within 1 of the oracle's (the rule and its reason: _compare)."""
    from planarslam_amd import Optimizer
    b, params, orc = pose_regime_run(name, mode)
    opt = Optimizer(params)
    got = (opt.PoseOptimization if mode == 0 else opt.TranslationOptimization)(b, 4, 10)
    want = golden_pose(pose_regimes, name, mode, b)
    print(f"pose regime {name} mode {mode}: device - reference {np.abs(got['Tcw'] - want['Tcw']).max():.2e}, oracle - reference "
          f"{np.abs(orc['Tcw'] - want['Tcw']).max():.2e}, lm_iters device {got['lm_iters'].tolist()} oracle {orc['lm_iters'].tolist()}")
    assert np.abs(got["Tcw"] - want["Tcw"]).max() <= POSE_TOL
    assert np.array_equal(got["n_inliers"], want["n_inliers"])
    for k in ("pt_outlier", "ln_outlier", "pl_outlier"):
        assert np.array_equal(got[k], want[k]), k
    assert np.abs(got["lm_iters"] - orc["lm_iters"]).max() <= 1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rounds,its", [(1, 1), (2, 3), (3, 10), (4, 1)])
def test_pose_protocol_sweep(mode, rounds, its):
    _compare(pose_batch(B=3, n_points=200, n_lines=20, n_planes=3, seed=57), mode, rounds=rounds, its=its)


def _contract_untouched(b, mode):
    """Entries that the contract of include/planar_abi.h leaves to the caller, stated from the batch alone: index at or above the frame's count, valid byte
    clear, parallel / vertical kinds in translation mode, every plane entry of a frame on which TranslationOptimization returns early."""
    MP, ML, MM = b["pt_valid"].shape[1], b["ln_valid"].shape[1], b["pl_valid"].shape[1]
    pt = (b["pt_valid"] == 0) | (np.arange(MP)[None] >= b["n_points"][:, None])
    ln = (b["ln_valid"] == 0) | (np.arange(ML)[None] >= b["n_lines"][:, None])
    pl = (b["pl_valid"] == 0) | (np.arange(MM)[None, :, None] >= b["n_planes"][:, None, None])
    if mode == 1:
        pl[:, :, 1:] = True
        pl[(~pt).sum(1) < 3] = True
    return dict(pt_outlier=pt, ln_outlier=ln, pl_outlier=pl)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["ragged", "few_edges", "planes_partly_missing"])
def test_pose_callers_values_survive(name, mode):
    """Flags are written only where valid: arrays that start as 0xA5 on both sides come back equal as a whole, and hold 0xA5 wherever the contract says so."""
    b = cases.POSE_REGIME_CASES[name][0]() if name in cases.POSE_REGIME_CASES else cases.POSE_CASES[name][0]()
    rc, got = run_host(b, TUM3, mode, fill=FILL)
    assert rc == 0
    want = ol.pose_optimize(b, TUM3, mode, out_fill=FILL)
    _same_as_oracle(got, want)
    for k, untouched in _contract_untouched(b, mode).items():
        assert untouched.any() and not untouched.all(), k
        assert (got[k][untouched] == FILL).all(), k
        assert np.isin(got[k][~untouched], (0, 1)).all(), k


def _three_frames():
    b = pose_batch(B=3, n_points=60, n_lines=10, n_planes=3, seed=61, max_points=64, max_lines=12, max_planes=4)
    b["pt_valid"][:] = 1; b["ln_valid"][:] = 1; b["pl_valid"][:] = 1          # padding included: a count read beyond its stride finds "valid" entries
    b["n_points"][:] = [50, 60, 50]; b["n_lines"][:] = [8, 10, 8]; b["n_planes"][:] = [2, 3, 0]
    return b


@pytest.mark.parametrize("mode", [0, 1])
def test_pose_counts_beyond_the_strides_are_clamped(mode):
    """Only the middle frame's point and line counts exceed their strides: it equals the oracle on the clamped counts, its neighbours equal the oracle and
    their rows hold no foreign write."""
    b = _three_frames()
    over = dict(b, n_points=b["n_points"].copy(), n_lines=b["n_lines"].copy())
    over["n_points"][1] = 64 + 5; over["n_lines"][1] = 12 + 3
    clamped = dict(b, n_points=b["n_points"].copy(), n_lines=b["n_lines"].copy())
    clamped["n_points"][1] = 64; clamped["n_lines"][1] = 12
    rc, got = run_host(over, TUM3, mode, fill=FILL)
    assert rc == 0
    want = ol.pose_optimize(clamped, TUM3, mode, out_fill=FILL)
    _same_as_oracle(got, want)
    for k, untouched in _contract_untouched(clamped, mode).items():
        assert (got[k][untouched] == FILL).all(), k
    neg = dict(b, n_points=np.array([50, -4, 50], np.int32), n_lines=np.array([8, -1, 8], np.int32), n_planes=np.array([2, -2, 0], np.int32))
    rc, got = run_host(neg, TUM3, mode, fill=FILL)
    assert rc == 0
    _same_as_oracle(got, ol.pose_optimize(dict(b, n_points=np.array([50, 0, 50], np.int32), n_lines=np.array([8, 0, 8], np.int32),
                                               n_planes=np.array([2, 0, 0], np.int32)), TUM3, mode, out_fill=FILL))
    assert got["n_inliers"][1] == 0 and np.array_equal(got["Tcw"][1], b["Tcw"][1])
    assert (got["pt_outlier"][1] == FILL).all() and (got["ln_outlier"][1] == FILL).all() and (got["pl_outlier"][1] == FILL).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_pose_too_many_planes_is_refused_per_frame(mode):
    """Only the middle frame has more planes than the stride: -1, its pose copied, no plane flag of any frame touched by it (the last frame has no planes
    of its own, so its plane row must come back as given)."""
    b = _three_frames()
    over = dict(b, n_planes=np.array([2, 4 + 1, 0], np.int32))
    rc, got = run_host(over, TUM3, mode, fill=FILL)
    assert rc == 0
    assert got["n_inliers"][1] == -1 and got["lm_iters"][1] == 0 and np.array_equal(got["Tcw"][1], b["Tcw"][1])
    assert (got["pl_outlier"][1] == FILL).all() and (got["pl_outlier"][2] == FILL).all()
    assert (got["pt_outlier"][1, :60] == 0).all() and (got["pt_outlier"][1, 60:] == FILL).all()        # as an early return leaves them
    assert (got["ln_outlier"][1, :10] == 0).all() and (got["ln_outlier"][1, 10:] == FILL).all()
    want = ol.pose_optimize(b, TUM3, mode, out_fill=FILL)
    keep = [0, 2]
    assert np.abs(got["Tcw"][keep] - want["Tcw"][keep]).max() <= POSE_TOL
    for k in ("n_inliers", "pt_outlier", "ln_outlier", "pl_outlier"):
        assert np.array_equal(got[k][keep], want[k][keep]), k
    both = ol.pose_optimize(over, TUM3, mode, out_fill=FILL)                                           # the oracle follows the same rule
    for k in ("n_inliers", "pt_outlier", "ln_outlier", "pl_outlier"):
        assert np.array_equal(got[k], both[k]), k


def test_pose_refuses_what_does_not_fit_the_lds():
    """max_points = 140 000 with 32 planes needs more than 160 KiB of LDS per frame: PLANAR_EINVAL, nothing launched, outputs as given."""
    b = pose_batch(B=1, n_points=20, n_lines=4, n_planes=2, seed=63, max_points=140000, max_lines=8, max_planes=32)
    rc, got = run_host(b, TUM3, 0, fill=FILL)
    assert rc == EINVAL
    assert (got["pt_outlier"] == FILL).all() and (got["pl_outlier"] == FILL).all() and (got["n_inliers"] == -77).all() and not got["Tcw"].any()


def test_pose_argument_checks():
    small = pose_batch(B=2, n_points=40, n_lines=6, n_planes=2, seed=65)
    assert run_host(small, TUM3, 0)[0] == 0
    assert run_host(pose_batch(B=1, n_points=20, n_lines=4, n_planes=2, seed=63, max_planes=33), TUM3, 0)[0] == EINVAL
    for rounds, its, mode in ((0, 10, 0), (5, 10, 0), (4, 0, 0), (4, 10, 2), (4, 10, -1)):
        rc, got = run_host(small, TUM3, mode, rounds=rounds, its=its, fill=FILL)
        assert rc == EINVAL and (got["pt_outlier"] == FILL).all() and (got["n_inliers"] == -77).all(), (rounds, its, mode)

    def no_obs(pb):
        pb.pt_obs = None
    assert run_host(small, TUM3, 0, patch=no_obs)[0] == EINVAL


@pytest.mark.parametrize("mode", [0, 1])
def test_pose_without_lm_iters(mode):
    b = cases.POSE_CASES["ragged"][0]()
    rc0, full = run_host(b, TUM3, mode, fill=FILL)
    rc1, bare = run_host(b, TUM3, mode, fill=FILL, want_lm_iters=False)
    assert rc0 == 0 and rc1 == 0 and (bare["lm_iters"] == -77).all() and (full["lm_iters"] >= 0).all()
    for k in _OUT[:5]:
        assert np.array_equal(full[k], bare[k]), k


@pytest.mark.parametrize("mode", [0, 1])
def test_pose_device_entry_equals_host_entry(mode):
    """planar_pose_opt_dev on device arrays (torch tensors on the current stream) against planar_pose_opt: every output bit for bit."""
    import torch
    from planarslam_amd import Optimizer
    from planarslam_amd._lib import Context
    b = {k: np.ascontiguousarray(v) for k, v in cases.POSE_CASES["ragged"][0]().items()}
    rc, want = run_host(b, TUM3, mode, fill=FILL)
    assert rc == 0
    dev = torch.device("cuda", 0)
    d_in = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k != "T_gt"}
    d_out = {k: torch.from_numpy(v).to(dev) for k, v in _outputs(b, FILL).items()}
    opt = Optimizer(TUM3, Context(0, stream=torch.cuda.current_stream().cuda_stream))
    pb = _pose_batch_struct(d_in, d_out, lambda t: t.data_ptr())
    opt.enqueue_dev(pb, mode, 4, 10)
    torch.cuda.synchronize()
    for k in _OUT:
        assert np.array_equal(d_out[k].cpu().numpy(), want[k]), k
