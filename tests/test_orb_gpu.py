"""GPU parity tests (run with -m gpu on the MI355X box): the HIP ORB path through the C ABI against
(a) the CPU oracle on seeded inputs, stage by stage, and (b) the committed outputs of the REAL
reference ORBextractor (tests/golden).  Bit-exact: integer/byte work, and float fields that are
produced by the same IEEE operation sequence."""
import glob
import os

import numpy as np
import pytest

import oracle_lib as ol
import orb_cases as oc
from planarslam_amd.synth import gray_image

pytestmark = pytest.mark.gpu

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orb_*.npz")))


def _mk(W, H, B=1, nfeatures=1000, scale=1.2, nlevels=8, ini=20, mn=7):
    from planarslam_amd import ORBextractor
    return ORBextractor(nfeatures, scale, nlevels, ini, mn, width=W, height=H, max_batch=B)


@pytest.mark.parametrize("path", GOLD, ids=lambda p: os.path.basename(p)[4:-4])
def test_hip_matches_reference_golden(path):
    z = np.load(path)
    p = z["params"]
    img = z["image"]
    ex = _mk(img.shape[1], img.shape[0], 1, int(p[0]), float(p[1]), int(p[2]), int(p[3]), int(p[4]))
    kps, desc = ex(img)
    assert len(kps) == len(z["kps"])
    assert kps.tobytes() == z["kps"].tobytes()
    assert np.array_equal(desc, z["desc"])


def _assert_stages(ex, img, ref):
    """One frame through `ex`, stage by stage against the oracle's outputs `ref` (orb_cases.Facts): every pyramid level, every level's FAST candidates in the
    reference's emission order, every blurred level the oracle made, the keypoint fields and the descriptors.  Bit-exact."""
    from planarslam_amd._lib import check
    nlevels = len(ref.levels)
    assert ex.nlevels == nlevels
    kps, desc = ex(img)
    check(ex.L.planar_orb_check(ex.h))
    for l in range(nlevels):
        assert np.array_equal(ex.read_level(0, l), ref.levels[l]), f"pyramid level {l}"
    for l in range(nlevels):
        assert np.array_equal(ex.read_candidates(0, l), ref.cand[l]), f"FAST candidates level {l}"
    for l in range(nlevels):
        ob = ref.blurred[l]
        if ob is not None:
            assert np.array_equal(ex.read_level(0, l, blurred=True), ob), f"blur level {l}"
    assert len(kps) == len(ref.kps)
    for f in ("x", "y", "octave", "response", "size"):
        assert np.array_equal(kps[f], ref.kps[f]), f
    assert np.array_equal(kps["angle"], ref.kps["angle"])
    assert np.array_equal(desc, ref.desc)
    return kps, desc


@pytest.mark.parametrize("seed,W,H", [(1234, 640, 480), (77, 640, 480), (5, 400, 304), (9, 333, 257)])
def test_hip_stages_match_oracle(seed, W, H):
    # seed 77: heavy texture, tens of thousands of FAST candidates, deep octree
    img = oc.noisy(seed, W, H, 40) if seed == 77 else gray_image(seed, W, H)
    _assert_stages(_mk(W, H), img, oc.oracle_facts(img, oc.DEFAULTS))


@pytest.mark.parametrize("name", oc.NAMES)
def test_hip_stages_match_oracle_over_cases(name):
    """The table of tests/orb_cases.py (each case pinned to the real ORBextractor by tests/test_oracle_orb.py): wide frames with 2 .. 42 initial nodes (path_code's
    nIni branch), 32 code bits, 4 nIni kept keys per level, x above 4000 in the 12-bit field, 1 .. 12 levels, scale 1.1 .. 2, every threshold regime, cells of one
    tile and of 53 x 53 pixels."""
    ref = oc.facts(name)
    img, p = ref.image, oc.BY_NAME[name].params
    ex = _mk(img.shape[1], img.shape[0], 1, **p)
    kps, desc = _assert_stages(ex, img, ref)
    assert kps.tobytes() == ref.kps.tobytes()               # class_id included


def test_hip_batch_equals_single_and_is_deterministic():
    imgs = np.stack([gray_image(100 + i) for i in range(5)])
    ex = _mk(640, 480, B=8)
    res1 = ex(imgs)
    res2 = ex(imgs[::-1].copy())[::-1]
    o = ol.OrbOracle()
    for b in range(5):
        okps, odesc = o.extract(imgs[b])
        for res in (res1, res2):
            assert res[b][0].tobytes() == okps.tobytes()
            assert np.array_equal(res[b][1], odesc)


def test_hip_uniform_noise_worst_case_candidates():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (480, 640)).astype(np.uint8)
    o = ol.OrbOracle()
    okps, odesc = o.extract(img)
    kps, desc = _mk(640, 480)(img)
    assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc)


def test_hip_flat_image_has_no_keypoints():
    img = np.full((480, 640), 128, np.uint8)
    kps, desc = _mk(640, 480)(img)
    assert len(kps) == 0 and desc.shape == (0, 32)


def _same(res, kps, desc):
    return res[0].tobytes() == kps.tobytes() and np.array_equal(res[1], desc)


def test_batch_through_the_xcd_swizzle():
    """xcd_frame_block (common.h) deals the workgroups of orb_fast_cells, orb_blur and orb_describe to frames in groups of eight and keeps the plain order for the
    last B % 8 frames: B = 11 runs both branches in one launch, B = 8 and B = 16 the swizzled one alone.  Distinct frames, so a workgroup that took another
    frame's cell, tile or keypoints shows."""
    W, H, p = 160, 120, dict(nfeatures=300, scale=1.2, nlevels=3, ini=20, mn=7)
    imgs = np.stack([oc.noisy(200 + i, W, H, 25) for i in range(16)])
    imgs[4] = 128
    imgs[9] = oc.uniform(9, W, H)
    o = ol.OrbOracle(**p)
    want = [o.extract(im) for im in imgs]
    assert len(want[4][0]) == 0 and len({w[0].tobytes() for w in want}) == 16
    ex = _mk(W, H, B=16, **p)
    for B in (11, 8, 16):
        fwd = ex(imgs[:B])
        rev = ex(imgs[:B][::-1].copy())[::-1]
        for b in range(B):
            assert _same(fwd[b], *want[b]), f"B = {B}, frame {b}"
            assert _same(rev[b], *want[b]), f"B = {B} reversed, frame {b}"


def test_padded_rows_and_frame_stride():
    """orb_copy_level0 with pitch > W and a frame stride that is no multiple of the pitch, through the host entry point and through extract_dev on a torch
    buffer: the padding (all 255) must not reach level 0."""
    import ctypes as C
    import torch
    from planarslam_amd._lib import KP_DTYPE, check, lib
    W, H, B = 333, 257, 3
    pitch = W + 13
    stride = pitch * (H + 2) + 5
    imgs = np.stack([oc.noisy(300 + i, W, H, 25) for i in range(B)])
    o = ol.OrbOracle()
    want = [o.extract(im) for im in imgs]
    ex = _mk(W, H, B=B)
    plain = ex(imgs)
    buf = np.full(B * stride, 255, np.uint8)
    for b in range(B):
        buf[b * stride:b * stride + pitch * H].reshape(H, pitch)[:, :W] = imgs[b]
    cap = ex.kp_cap
    kps = np.zeros((B, cap), KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); n = np.zeros(B, np.int32)
    check(lib().planar_orb_extract(ex.h, buf.ctypes.data, B, pitch, stride, kps.ctypes.data, desc.ctypes.data, n.ctypes.data))
    for b in range(B):
        assert np.array_equal(ex.read_level(b, 0), imgs[b]), f"level 0 of frame {b}"
    host = [(kps[b, :n[b]], desc[b, :n[b]]) for b in range(B)]
    dev = torch.device("cuda:0")
    d_buf = torch.from_numpy(buf).to(dev)
    d_kps = torch.zeros(B * cap * KP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_dev(d_buf.data_ptr(), d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), B, pitch=pitch, frame_stride=stride)
    check(ex.L.planar_orb_check(ex.h))                      # waits for the extractor's stream
    torch.cuda.synchronize()
    tn = d_n.cpu().numpy()
    tk = d_kps.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    td = d_desc.cpu().numpy().reshape(B, cap, 32)
    for b in range(B):
        assert _same(plain[b], *want[b]), f"unpadded, frame {b}"
        assert _same(host[b], *want[b]), f"padded host buffer, frame {b}"
        assert _same((tk[b, :tn[b]], td[b, :tn[b]]), *want[b]), f"padded device buffer, frame {b}"


def test_extractor_reuse_leaves_no_state():
    """The per-cell, per-level and kept counts live in buffers that one extractor reuses between calls, and orb_octree returns early for a level without
    candidates: a dense frame, an empty one, a frame whose level 0 alone is empty, a textured one - each as from a fresh extractor."""
    W, H = 400, 304
    frames = [("noise", oc.uniform(31, W, H)), ("flat", np.full((H, W), 128, np.uint8)), ("checker_ties", oc.facts("checker_ties").image),
              ("textured", oc.noisy(32, W, H, 25))]
    o = ol.OrbOracle()
    ex = _mk(W, H)
    for name, img in frames:
        okps, odesc = o.extract(img)
        got = ex(img)
        assert _same(got, okps, odesc), f"reused extractor, {name}"
        assert _same(_mk(W, H)(img), okps, odesc), f"fresh extractor, {name}"
        for l in range(8):
            assert np.array_equal(ex.read_candidates(0, l), o.candidates(l)), f"{name}: candidates of level {l}"
        if name == "flat":
            assert len(got[0]) == 0 and got[1].shape == (0, 32)


@pytest.mark.parametrize("W,H,kw", [
    (240, 640, {}),                          # width / height rounds to 0 initial nodes: the reference divides by zero there
    (63, 64, {}), (4097, 128, {}),
    (640, 480, dict(nlevels=0)), (640, 480, dict(nlevels=17)),
    (64, 64, dict(nlevels=2)),               # level 1 (53 x 53) has no 30-pixel cell
    (640, 480, dict(scale=1.0)),
    (640, 480, dict(ini=7, mn=8)),
    (640, 480, dict(nfeatures=60001)),
], ids=["nIni0", "w63", "w4097", "levels0", "levels17", "level_without_cell", "scale1", "ini_below_min", "nfeatures60001"])
def test_create_refuses_what_it_cannot_do(W, H, kw):
    from planarslam_amd import PlanarError
    from planarslam_amd._lib import lib
    with pytest.raises(PlanarError):
        _mk(W, H, **kw)
    assert lib().planar_last_error()                        # a message, not only a code
    img = oc.facts("small_64").image                        # and the next valid extractor works
    kps, desc = _mk(64, 64, 1, **oc.BY_NAME["small_64"].params)(img)
    assert _same((kps, desc), oc.facts("small_64").kps, oc.facts("small_64").desc)


def test_errors_are_reported_not_raised_from_c():
    from planarslam_amd import PlanarError
    with pytest.raises(PlanarError):
        _mk(32, 32)                       # below the supported size
    ex = _mk(640, 480)
    with pytest.raises(ValueError):
        ex(np.zeros((100, 100), np.uint8))
    with pytest.raises(TypeError):
        ex(np.zeros((480, 640), np.float32))
