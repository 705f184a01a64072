"""The targets of the device tree build's tests (tests/test_forest_device_abi.py checks their fixture conditions on the host,
tests/test_gpu_forest_device.py builds them on the GPU). Plain data from fixed seeds; nothing here needs a device."""
import ctypes

import numpy as np

# What locgpu_icp_device_build_info reports (csrc/forest_build.hpp: kFbTile, kFbLaneLen); the GPU test asserts that it still does, so
# that the sizes below stay one below, at and above each threshold.
TILE, LANE_LEN = 256, 32
SIZES = (1, 2, 3, 5, 63, 64, 65, LANE_LEN - 1, LANE_LEN, LANE_LEN + 1, TILE - 1, TILE, TILE + 1, 2049, 4000)
OFFSET_NAME = "offset"


def _normal(seed, n, sigma=20.0):
    return np.random.default_rng(seed).normal(0.0, sigma, (n, 3)).astype(np.float32)


def line_y(n=301):
    """On a line along y: the x and z variances are exactly zero."""
    c = np.zeros((n, 3), np.float32)
    c[:, 0] = 1.5
    c[:, 1] = (0.37 * ((np.arange(n) * 97) % n)).astype(np.float32)
    c[:, 2] = -2.0
    return c


def tie_xy(n=500):
    """y = x point for point: the x and y variances are the same float at every node, so the strict > keeps axis 0."""
    r = np.random.default_rng(77)
    v = r.normal(0.0, 5.0, n).astype(np.float32)
    return np.stack([v, v, (0.1 * r.normal(0.0, 1.0, n)).astype(np.float32)], axis=1)


def offset(n=4000):
    """About 5000 m from the origin: every float32 sum of the top levels rounds."""
    c = _normal(80, n)  # a seed at which numpy's pairwise sum and the index-order sum differ on both x and y (test_forest_device_abi.py asserts it)
    c[:, 0] += 5000.0
    c[:, 1] -= 5000.0
    c[:, 2] *= 0.1
    return c


def tiny(n=777):
    """Scaled by 1e-22: the squared deviations are float32 subnormals."""
    return (_normal(79, n).astype(np.float64) * 1e-22).astype(np.float32)


def local_map(synth, n=20000):
    return np.ascontiguousarray(synth.make_local_map(n, 14, half=30.0)[:, :3])


def forest_targets(synth):
    """[(name, cloud [n, 3] float32)]: the size cases, the local map and the special trees — one forest."""
    out = [("n%d" % n, _normal(100 + n, n)) for n in SIZES]
    out.append(("local_map", local_map(synth)))
    out += [("line_y", line_y()), ("tie_xy", tie_xy()), (OFFSET_NAME, offset()), ("tiny", tiny())]
    assert {len(c) % 2 for _, c in out} == {0, 1}
    return out


def pair_world(synth):
    """Six consecutive scans of unequal counts and seven targets (five of the scans, a local map in scan 4's frame, five points)."""
    sids, counts = (10, 11, 12, 13, 14, 15), (4000, 3100, 2049, 1500, 900, 257)
    scans = [np.ascontiguousarray(synth.make_scan(s, subsample=n)[:, :3]) for s, n in zip(sids, counts)]
    _, init4 = synth.make_pose(sids[4])
    x, y, z, w = init4[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    m = synth.make_local_map(20000, sids[4], half=30.0)
    local = np.ascontiguousarray(((m[:, :3].astype(np.float64) - init4[4:]) @ R).astype(np.float32))
    return dict(scans=scans, targets=scans[:5] + [local, np.ascontiguousarray(scans[5][:5])], target_of=(-1, 0, 1, 2, 5, 6))


def single_clouds(synth):
    return [_normal(357, 257), local_map(synth)]


def with_duplicate():
    """Three scans; point 7 of scan 1 is point 8 again: one degenerate split in tree 1."""
    scans = [_normal(400, 300), _normal(401, 1000), _normal(402, 65)]
    scans[1][7] = scans[1][8]
    return scans


def with_huge():
    """Two scans; one coordinate of scan 1 is 1e19: squared distances to it overflow, the fast search kernel must stay off."""
    scans = [_normal(410, 300), _normal(411, 500)]
    scans[1][9, 1] = 1e19
    return scans


def deep_chain(m=24, ratio=60.0, first=1e-15):
    """3 m = 72 points, m on each axis at first * ratio^i: nearly every split peels one point off, the tree is deeper than 64 levels."""
    pts = np.zeros((3 * m, 3), dtype=np.float32)
    for a in range(3):
        pts[a * m:(a + 1) * m, a] = (first * ratio ** np.arange(m, dtype=np.float64)).astype(np.float32)
    return pts


def host_tree(api, xyz):
    """(slots uint64, info = [leaves, nodes, depth]) of the host builder for one cloud (locgpu_debug_build_tree); needs no device."""
    L = api.lib()
    L.locgpu_debug_build_tree.restype = ctypes.c_size_t
    L.locgpu_debug_build_tree.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    info = np.zeros(3, dtype=np.int64)
    n = L.locgpu_debug_build_tree(xyz.ctypes.data, len(xyz), None, 0, info.ctypes.data)
    slots = np.zeros(n, dtype=np.uint64)
    L.locgpu_debug_build_tree(xyz.ctypes.data, len(xyz), slots.ctypes.data, n, info.ctypes.data)
    return slots, info
