"""Inputs and the CPU reference of the global-map tests (locgpu_clouds_merge / locgpu_batch_merge; Lio::GetGlobalMap, lio.cpp:550-614).

The reference is built from three oracle calls and nothing of the library under test:
  locref.transform_cloud_f64 per cloud  →  np.concatenate  →  locref.voxel_grid(joined, all_dense, leaf, SORT_STABLE, with_info=True).
tests/test_gpu_filters.py establishes byte equality between the device filter and that oracle call on its own."""
import numpy as np

BLOCK = 256  # kMB of csrc/cloud_merge.hip: output points per block of the transform-and-join launch

# point counts per cloud: the first straddles the block (255 | 256 | 257) behind an empty first cloud; the other two put two empty
# clouds in a row (in the middle, and at the very start) and an empty cloud last
LAYOUTS = {
    "straddle": [0, 1, 255, 256, 257, 1000, 3],
    "empty_pair": [300, 0, 0, 613, 2, 0],
    "empty_ends": [0, 0, 256, 0, 0, 700, 0],
}
LEAVES = (0.0, 0.5, 2.0, 1e-4)
PATCH = 20.0  # metres: the side of the ground patch


def make_poses(n, seed=11):
    """n poses (quaternion xyzw + translation): a real rotation about a tilted axis, translations of up to 2 m."""
    rng = np.random.default_rng(seed)
    axis = np.array([0.25, -0.15, 1.0])
    axis /= np.linalg.norm(axis)
    poses = np.zeros((n, 7))
    for k in range(n):
        ang = 0.15 + 0.11 * k
        poses[k, :3] = axis * np.sin(0.5 * ang)
        poses[k, 3] = np.cos(0.5 * ang)
        poses[k, 4:] = rng.uniform(-2.0, 2.0, 3)
    return poses


def make_clouds(counts, seed=5):
    """(clouds [n_i, 4] float32, dense flags): points on the ground patch with intensities set. The largest cloud is NOT flagged dense
    and holds a NaN, an Inf and an all-NaN point."""
    rng = np.random.default_rng(seed)
    clouds, dense = [], []
    for n in counts:
        c = np.zeros((n, 4), np.float32)
        c[:, 0:2] = rng.uniform(-0.5 * PATCH, 0.5 * PATCH, (n, 2))
        c[:, 2] = rng.normal(0.0, 0.05, n)
        c[:, 3] = rng.uniform(0.0, 255.0, n)
        clouds.append(c)
        dense.append(True)
    big = int(np.argmax(counts))
    assert counts[big] >= 600
    clouds[big][17, 1] = np.nan
    clouds[big][300, 0] = np.inf
    clouds[big][599, :3] = np.nan
    dense[big] = False
    return clouds, dense


def transformed(locref, clouds, dense, poses):
    if poses is None:
        return [c.copy() for c in clouds]
    return [locref.transform_cloud_f64(p, c, d) if len(c) else c.copy() for c, d, p in zip(clouds, dense, poses)]


def reference(locref, clouds, dense, poses, leaf):
    """(points [m, 4] float32, is_dense, passthrough) of GetGlobalMap on the oracle."""
    joined = np.ascontiguousarray(np.concatenate(transformed(locref, clouds, dense, poses)), dtype=np.float32).reshape(-1, 4)
    all_dense = all(dense)  # a fresh pcl::PointCloud is dense; operator+= ANDs the flags, those of empty clouds too
    if leaf == 0:
        return joined, all_dense, False
    out, info = locref.voxel_grid(joined, all_dense, leaf, order=locref.SORT_STABLE, with_info=True)
    # applyFilter sets output.is_dense; its "leaf size is too small" pass-through copies the input, flag included
    return out, (all_dense if info["status"] == 1 else True), info["status"] == 1


def shared_voxels(locref, clouds, dense, poses, leaf):
    """(voxels that hold finite points of two or more clouds, voxels) at `leaf`, in VoxelGrid's own float32 index arithmetic."""
    parts = transformed(locref, clouds, dense, poses)
    pts = np.concatenate(parts)
    owner = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    ok = np.isfinite(pts[:, :3]).all(axis=1)
    pts, owner = pts[ok], owner[ok]
    inv = np.float32(1.0) / np.float32(leaf)
    ijk = np.floor(pts[:, :3] * inv).astype(np.int64)
    ijk -= ijk.min(axis=0)
    div = ijk.max(axis=0) + 1
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    pairs = np.unique(np.stack([idx, owner], axis=1), axis=0)
    _, per_voxel = np.unique(pairs[:, 0], return_counts=True)
    return int((per_voxel >= 2).sum()), int(len(per_voxel))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
