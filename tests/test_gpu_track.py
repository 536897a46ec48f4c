"""GPU: argus_roi_from_pose (csrc/track.hip) against its fp64 restatement (tests/track_reference.py) on the shared
case set: 4096 poses (degenerate ones among them) through two cameras, with and without jitter, an index and
smoothing; validity, the home fallback, ``used``, check_roi's domain, complete writes, untouched guard words, the
group and workgroup edges, null outputs, the index clamp, and bit-reproducibility.

The tolerance is track_reference.TOL_PX = 2^-7 px: five times the distance of the restatement evaluated in fp32 from
the one evaluated in fp64 on this set (tests/test_track_host.py prints and bounds it)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import track_reference as ref  # noqa: E402

from argus_amd.pose_session import check_roi  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64  # float / int32 words behind every output


@pytest.fixture(scope="module")
def cases():
    return ref.case_set()


def _cfg(smooth=1.0, scale=(0.25, 4.0)):
    from argus_amd._lib import TrackCfg

    return TrackCfg((C.c_float * 3)(*ref.HALF_EXTENT), ref.MARGIN, scale[0], scale[1], ref.Z_NEAR, smooth)


def _launch(cuda, poses, cams, batch, *, index=None, jitter=None, home=None, prev=None, smooth=1.0, used=True,
            valid=True, n_poses=None):
    """One launch on NaN-prefilled outputs with guard words behind each buffer. Returns numpy (rois, used or None,
    valid or None) after checking the guards."""
    from argus_amd._lib import lib, ptr, stream

    n = batch * len(cams)
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(cuda)  # noqa: E731
    dposes, dcams = dev(poses, torch.float32), dev(cams, torch.float32)
    home = ref.center_home(n) if home is None else home
    dhome = dev(home, torch.float32)
    rois = torch.full((4 * n + GUARD,), float("nan"), dtype=torch.float32, device=cuda)
    rois[:4 * n] = dev(home if prev is None else prev, torch.float32).reshape(-1)  # previous in, next out
    rois[4 * n:] = 12345.0
    dused = torch.full((4 * n + GUARD,), float("nan"), dtype=torch.float32, device=cuda)
    dused[4 * n:] = 12345.0
    dvalid = torch.full((n + GUARD,), -7, dtype=torch.int32, device=cuda)
    dindex = None if index is None else dev(index, torch.int64)
    djit = None if jitter is None else dev(jitter, torch.float32)
    cfg = _cfg(smooth)
    lib().roi_from_pose(batch, len(cams), *ref.FRAME_HW, *ref.HW, ptr(dposes), len(poses) if n_poses is None else n_poses,
                        ptr(dindex), ptr(dcams), C.byref(cfg), ptr(djit), ptr(dhome), ptr(rois),
                        ptr(dused) if used else None, ptr(dvalid) if valid else None, stream())
    torch.cuda.synchronize()
    assert bool((rois[4 * n:] == 12345.0).all()) and bool((dused[4 * n:] == 12345.0).all())
    assert bool((dvalid[n:] == -7).all())
    if not used:
        assert bool(torch.isnan(dused[:4 * n]).all())
    if not valid:
        assert bool((dvalid[:n] == -7).all())
    return (rois[:4 * n].view(n, 4).cpu().numpy(), dused[:4 * n].view(n, 4).cpu().numpy() if used else None,
            dvalid[:n].cpu().numpy() if valid else None)


def _want(poses, cams, **kw):
    return ref.roi_from_pose(poses, cams, ref.FRAME_HW, ref.HW, ref.HALF_EXTENT, ref.MARGIN, ref.Z_NEAR, **kw)


def _check(got, want, home, prev):
    rois, used, valid = got
    n = len(rois)
    assert np.isfinite(rois).all()  # the NaN prefill is gone: every region written
    check_roi(torch.from_numpy(rois).reshape(n, 1, 4), ref.FRAME_HW, ref.HW)  # raises on any violation
    assert np.array_equal(valid, want["valid"])
    bad = valid == 0
    assert np.array_equal(rois[bad].view(np.uint32), home[bad].view(np.uint32))  # home, bit for bit
    assert np.array_equal(used.view(np.uint32), prev.view(np.uint32))
    err = np.abs(rois.astype(np.float64) - want["rois"].astype(np.float64))
    free = ~want["touched"]
    print(f"n {n}  valid {valid.mean():.3f}  unclamped {free.mean():.3f}  largest |gpu - fp64| {err.max():.3e} px "
          f"(unclamped: {err[free].max() if free.any() else 0.0:.3e})")
    assert err.max() <= ref.TOL_PX
    return free.mean()


@pytest.mark.parametrize("smooth", [1.0, 0.3])
@pytest.mark.parametrize("indexed", [False, True], ids=["direct", "indexed"])
@pytest.mark.parametrize("jittered", [False, True], ids=["plain", "jitter"])
def test_kernel_matches_the_fp64_restatement_on_the_case_set(cuda, cases, smooth, indexed, jittered):
    poses, cams, jit = cases
    n = 2 * ref.N_POSES
    index = np.random.RandomState(5).permutation(ref.N_POSES).astype(np.int64) if indexed else None
    jitter = jit if jittered else None
    home = ref.center_home(n)
    home[::3] = np.float32([3.5, 70.25, 40.0, 80.0])  # not every home is the center crop
    prev = home.copy()
    prev[1::2] = np.float32([20.0, 10.5, 50.0, 50.0])
    got = _launch(cuda, poses, cams, ref.N_POSES, index=index, jitter=jitter, home=home, prev=prev, smooth=smooth)
    want = _want(poses, cams, index=index, jitter=jitter, home=home, prev=prev, smooth=smooth)
    share = _check(got, want, home, prev)
    assert share >= 0.25  # the parity is not carried by clamped values
    again = _launch(cuda, poses, cams, ref.N_POSES, index=index, jitter=jitter, home=home, prev=prev, smooth=smooth)
    for a, b in zip(got, again):  # two runs, identical bits
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n_cams,batch", [(1, 1), (3, 1), (1, 31), (1, 32), (2, 16), (1, 33), (3, 11), (2, 33), (3, 22)],
                         ids=lambda v: str(v))
def test_group_and_workgroup_edges(cuda, cases, n_cams, batch):
    """batch * n_cams in {1, 3, 31, 32, 33, 66}: one group, a partial and a full workgroup, one image into the next
    workgroup, two full workgroups and a bit."""
    poses, cams2, jit = cases
    third = ref.look_at_camera((0.17, 0.0, 0.12), (0, 0, 0), 70.0, ref.FRAME_HW)
    cams = np.concatenate([cams2, third[None]])[:n_cams]
    p = poses[100:100 + batch]  # ordinary poses
    n = batch * n_cams
    assert n in (1, 3, 31, 32, 33, 66)
    home = ref.center_home(n)
    prev = home.copy()
    prev[:, 0] += np.arange(n, dtype=np.float32) / 4  # every image has a previous region of its own
    got = _launch(cuda, p, cams, batch, jitter=jit[:n], home=home, prev=prev, smooth=0.5)
    want = _want(p, cams, jitter=jit[:n], home=home, prev=prev, smooth=0.5)
    _check(got, want, home, prev)


def test_null_used_and_valid(cuda, cases):
    poses, cams, _ = cases
    full = _launch(cuda, poses[:40], cams, 40)
    for used, valid in ((False, True), (True, False), (False, False)):
        got = _launch(cuda, poses[:40], cams, 40, used=used, valid=valid)
        assert np.array_equal(got[0].view(np.uint32), full[0].view(np.uint32))
        assert (got[1] is None) == (not used) and (got[2] is None) == (not valid)


def test_out_of_range_index_clamps(cuda, cases):
    poses, cams, _ = cases
    index = np.array([-1, -(1 << 40), 200, 299, 300, 1 << 40, 150], dtype=np.int64)
    got = _launch(cuda, poses, cams, len(index), index=index, n_poses=300)  # the table ends at 300
    want = _launch(cuda, poses, cams, len(index), index=np.array([0, 0, 200, 299, 299, 299, 150], dtype=np.int64))
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ref_ = _want(poses[:300], cams, index=index)
    assert np.array_equal(got[2], ref_["valid"]) and np.abs(got[0] - ref_["rois"]).max() <= ref.TOL_PX


def test_any_pose_bits_give_a_served_region(cuda):
    """The memory-safety argument: random BIT PATTERNS as poses (NaNs, infinities, denormals, 1e38) still give
    regions inside check_roi's domain, or home."""
    rng = np.random.RandomState(17)
    bits = rng.randint(0, 1 << 32, size=(2048, 7), dtype=np.uint64).astype(np.uint32)
    poses = bits.view(np.float32)
    cams = ref.case_set()[1]
    rois, _, valid = _launch(cuda, poses, cams, 2048)
    check_roi(torch.from_numpy(rois).reshape(-1, 1, 4), ref.FRAME_HW, ref.HW)
    home = ref.center_home(4096)
    assert np.array_equal(rois[valid == 0], home[valid == 0]) and (valid == 0).any()
