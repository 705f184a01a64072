"""Conditions on the INPUTS of the global-map tests (tests/global_map_ref.py), checked on the CPU oracle alone: without them the GPU
tests of locgpu_clouds_merge could pass for the wrong reason.
  - voxels are shared between clouds, so the filter really merges points of different clouds;
  - joining the clouds in another order changes the output bytes, so a test of the join order is sensitive;
  - leaf 1e-4 reaches PCL's "leaf size is too small" pass-through."""
import numpy as np
import pytest

import global_map_ref as gm


@pytest.fixture(scope="module")
def world():
    counts = gm.LAYOUTS["straddle"]
    clouds, dense = gm.make_clouds(counts)
    return clouds, dense, gm.make_poses(len(counts))


def test_layouts_are_what_the_kernel_can_get_wrong():
    a, b, c = (gm.LAYOUTS[k] for k in ("straddle", "empty_pair", "empty_ends"))
    assert a[0] == 0 and {gm.BLOCK - 1, gm.BLOCK, gm.BLOCK + 1} <= set(a) and sum(a) > 4 * gm.BLOCK
    for lay in (b, c):
        assert any(x == 0 and y == 0 for x, y in zip(lay, lay[1:])) and lay[-1] == 0 and sum(lay) > gm.BLOCK
    assert c[0] == 0 and c[1] == 0


def test_inputs_hold_what_they_claim(world):
    clouds, dense, poses = world
    assert dense.count(False) == 1
    big = clouds[dense.index(False)]
    bad = ~np.isfinite(big[:, :3])
    assert np.isnan(big[:, :3]).all(axis=1).sum() == 1 and np.isinf(big[:, :3]).sum() == 1 and bad.any(axis=1).sum() == 3
    for c in clouds:
        assert c.dtype == np.float32 and (len(c) == 0 or (np.ptp(c[:, 3]) > 0 or len(c) == 1))
        fin = c[np.isfinite(c[:, :3]).all(axis=1)]
        assert len(fin) == 0 or np.abs(fin[:, :2]).max() <= 0.5 * gm.PATCH
    assert np.abs(poses[:, 4:]).max() <= 2.0 and np.abs(poses[:, 4:]).max() > 0.5
    assert np.allclose(np.linalg.norm(poses[:, :4], axis=1), 1.0)
    assert (np.abs(poses[:, 0]) > 1e-3).all() and (np.abs(poses[:, 2]) > 1e-2).all()  # tilted axis, real angle


def test_voxels_are_shared_between_clouds(world, locref):
    clouds, dense, poses = world
    for leaf in (2.0, 0.5):
        shared, total = gm.shared_voxels(locref, clouds, dense, poses, leaf)
        out, is_dense, passthrough = gm.reference(locref, clouds, dense, poses, leaf)
        print("leaf %.1f: %d of %d voxels hold points of two or more clouds" % (leaf, shared, total))
        assert shared >= 1 and total == len(out) and is_dense and not passthrough


def test_join_order_changes_the_bytes(world, locref):
    clouds, dense, poses = world
    fwd, _, _ = gm.reference(locref, clouds, dense, poses, 2.0)
    rev, _, _ = gm.reference(locref, clouds[::-1], dense[::-1], poses[::-1], 2.0)
    assert fwd.shape == rev.shape  # the same voxels either way
    diff = np.abs(fwd - rev).max()
    print("reversed join order: largest difference %.3g" % diff)
    assert not np.array_equal(gm.bits(fwd), gm.bits(rev)) and diff < 1e-3


def test_small_leaf_reaches_the_passthrough(world, locref):
    clouds, dense, poses = world
    out, is_dense, passthrough = gm.reference(locref, clouds, dense, poses, 1e-4)
    joined, all_dense, _ = gm.reference(locref, clouds, dense, poses, 0.0)
    assert passthrough and not is_dense and not all_dense
    assert out.tobytes() == joined.tobytes() and len(out) == sum(len(c) for c in clouds)  # non-finite points included
    # without poses the reference carries the bits through
    raw, _, _ = gm.reference(locref, clouds, dense, None, 0.0)
    assert raw.tobytes() == np.concatenate(clouds).tobytes()
