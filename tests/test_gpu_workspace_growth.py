"""The workspaces and handles of the library only ever grow, and they grow by discarding what they held — except a resident cloud that
is appended to and the incremental NDT voxel set, which keep it. A steady-state test never reaches either path, so here every call
is made small, then large enough to outgrow the headroom the small call left (with_headroom(n) = n + n / 4 + 1024 points, n + 16
scans), then small again, all on ONE long-lived context — and each result must be, bit for bit, what the same call gives as the first
call of a fresh context."""
import numpy as np
import pytest

from test_gpu_loam_features import _scan as _ring_scan

pytestmark = pytest.mark.gpu


def _headroom(n):
    return n + n // 4 + 1024


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a == b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cloud(n, seed, with_nan=False):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    c[:, 3] = (np.arange(n) % 251).astype(np.float32)
    if with_nan:
        c[::7, 1] = np.nan
    return c


def _rings(synth, rings, pts, scan_id=3):
    """The first `pts` points of the first `rings` rings of a synthetic scan (rows of 1800 points), ring after ring."""
    c, ring = _ring_scan(synth, scan_id)
    idx = (np.arange(rings)[:, None] * 1800 + np.arange(pts)[None, :]).ravel()
    return np.ascontiguousarray(c[idx]), np.ascontiguousarray(ring[idx])


def _small_large_small(api, call, small, large):
    """call(ctx, arg) → arrays. On one context: small, large, small; each against the first call of a fresh context."""
    want = []
    for arg in (small, large):
        fresh = api.Context(0)
        want.append(call(fresh, arg))
        fresh.close()
    ctx = api.Context(0)
    got = [call(ctx, small), call(ctx, large), call(ctx, small)]
    ctx.close()
    assert _same(got[0], want[0]), "small, first"
    assert _same(got[1], want[1]), "large, after the workspaces grew"
    assert _same(got[2], want[0]), "small again, in the grown workspaces"
    return want


# ---------------------------------------------------------------------------------------------- single clouds
@pytest.mark.parametrize("in_place", [True, False])
def test_voxel_filter_grows_its_scratch(api, in_place):
    assert _headroom(300 + 1) < 3000

    def call(ctx, pts):
        c = api.Cloud(ctx, pts)
        out = c.voxel_filter(0.7) if not in_place else c.voxel_filter(0.7, out=c)
        return out.download()

    want = _small_large_small(api, call, _cloud(300, 1), _cloud(3000, 2))
    assert 0 < len(want[0]) < 300 and len(want[0]) < len(want[1]) < 3000


def test_remove_nan_grows_its_scratch(api):
    def call(ctx, pts):
        return api.Cloud(ctx, pts, is_dense=False).remove_nan().download()

    want = _small_large_small(api, call, _cloud(300, 3, with_nan=True), _cloud(3000, 4, with_nan=True))
    assert len(want[0]) == 300 - len(range(0, 300, 7)) and len(want[1]) == 3000 - len(range(0, 3000, 7))


# (rings, points per ring): the first pair crosses the task and the point capacity with rings the picker skips (fewer than 131 points:
# both outputs are empty), the second with rings it works on
@pytest.mark.parametrize("small,large", [((16, 40), (32, 120)), ((16, 150), (32, 400))])
def test_cloud_loam_extract_grows_tasks_and_points(api, synth, small, large):
    assert _headroom(small[0] * small[1]) < large[0] * large[1] and small[0] < large[0]

    def call(ctx, shape):
        c, ring = _rings(synth, *shape)
        edge, surf = api.Cloud(ctx, c).loam_extract(ring, shape[0])
        return edge.download(), surf.download()

    want = _small_large_small(api, call, small, large)
    if small[1] >= 131:
        assert all(len(e) > 0 and len(s) > 0 for e, s in want)


def test_cloud_append_keeps_the_points_it_had(api):
    a, b = _cloud(300, 5), _cloud(3000, 6)
    ctx = api.Context(0)
    c = api.Cloud(ctx, a)
    assert _headroom(300) < 300 + 3000
    got = c.append(api.Cloud(ctx, b)).download()
    ctx.close()
    assert got.shape == (3300, 4) and _same(got[:300], a) and _same(got[300:], b)


# ---------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("in_place", [True, False])
def test_batch_preprocess_grows_scans_and_slots(api, in_place):
    assert 2 + 16 < 20 and _headroom(2 * 300) < 20 * 1500

    def call(ctx, shape):
        n_scans, n = shape
        scans = [_cloud(n - 3 * i, 100 + i, with_nan=True)[:, :3].copy() for i in range(n_scans)]
        src = api.Batch(ctx, scans)
        dst = src if in_place else api.Batch(ctx, None, n_scans=n_scans, max_points=n)
        counts, status = src.preprocess(0.9, out=None if in_place else dst)
        out = [dst.download_scan(i) for i in range(n_scans)]
        src.close()
        if not in_place:
            dst.close()
        return [counts, status] + out

    want = _small_large_small(api, call, (2, 300), (20, 1500))
    assert all(0 < c < 300 for c in want[0][0]) and all(0 < c < 1500 for c in want[1][0])


def test_batch_loam_extract_grows_scans_rings_and_slots(api, synth):
    small, large = (2, 4, 150), (20, 8, 200)  # scans, rings per scan, points per ring
    assert small[0] + 16 < large[0] and _headroom(small[0] * small[1] * small[2]) < large[0] * large[1] * large[2]
    assert small[0] * small[1] + small[0] * small[1] // 4 + 64 < large[0] * large[1]

    def call(ctx, shape):
        n_scans, rings, pts = shape
        scans, ring_arrays = [], []
        for i in range(n_scans):
            c, ring = _rings(synth, rings, pts, scan_id=i % 5)
            scans.append(np.ascontiguousarray(c[:, :3]))
            ring_arrays.append(ring)
        src = api.Batch(ctx, scans)
        edge = api.Batch(ctx, None, n_scans=n_scans, max_points=rings * pts)
        surf = api.Batch(ctx, None, n_scans=n_scans, max_points=rings * pts)
        ne, ns, status = src.loam_extract(ring_arrays, rings, edge, surf)
        out = [edge.download_scan(i) for i in range(n_scans)] + [surf.download_scan(i) for i in range(n_scans)]
        for b in (src, edge, surf):
            b.close()
        return [ne, ns, status] + out

    want = _small_large_small(api, call, small, large)
    assert all(int(w[0].sum()) > 0 and int(w[1].sum()) > 0 and not w[2].any() for w in want)


# ---------------------------------------------------------------------------------------------- matchers
def test_icp_align_grows_the_one_scan_batch(api, small_world):
    small, large = small_world["scan2k"][::8], small_world["scan10k"][::3]
    assert _headroom(len(small)) < len(large)
    opts = api.icp_opts(method=api.P2PLANE)

    def call(ctx, scan):
        if not getattr(ctx, "_has_target", False):
            ctx.icp_set_target(small_world["map"])
            ctx._has_target = True
        pose, st = ctx.icp_align(scan, small_world["init_pose"], opts)
        return pose, np.array([st["iterations"]])

    want = _small_large_small(api, call, small, large)
    assert all(int(w[1][0]) > 1 for w in want)


def test_loam_handle_reshapes_its_batches_and_joint_state(api, small_world):
    m, s2, s10 = small_world["map"], small_world["scan2k"], small_world["scan10k"]
    edge_map, surf_map = m[::20], m[::4]
    init = np.array(small_world["init_pose"], dtype=np.float64)
    one = (s2[::7], s2[np.arange(len(s2)) % 7 != 0])
    four = [(s10[i::28], s10[(np.arange(len(s10)) % 7 != 0) & (np.arange(len(s10)) % 4 == i)]) for i in range(4)]

    def scan_match(h):
        pose, st, cloud = h.scan_match(one[0], one[1], init)
        return pose, np.array([st["iterations"], st["status"]]), cloud

    def align_batch(h):
        poses, st = h.align_batch([f[0] for f in four], [f[1] for f in four], np.stack([init] * 4))
        return poses, np.array([[x["iterations"], x["status"]] for x in st])

    want = []
    for call in (scan_match, align_batch):
        h = api.Loam()
        h.set_target(edge_map, surf_map)
        want.append(call(h))
        h.close()
    h = api.Loam()
    h.set_target(edge_map, surf_map)
    got = [scan_match(h), align_batch(h), scan_match(h)]
    h.close()
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[0])
    assert want[0][1][0] > 1 and (want[1][1][:, 0] > 1).all()


# ---------------------------------------------------------------------------------------------- incremental NDT
def _voxel_cloud(x0, nx, ny, seed, per_voxel=4):
    """per_voxel points in each of the nx × ny unit voxels whose corner is (x0 + i, j, 0): well inside their voxel."""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2)
    base = np.concatenate([ij + np.array([x0, 0]), np.zeros((len(ij), 1))], 1) + 0.5
    pts = np.repeat(base, per_voxel, 0) + rng.uniform(-0.3, 0.3, (len(ij) * per_voxel, 3))
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], dtype=np.float32), len(ij)


def _rows_of(dump, keys):
    """The dump's (mu, info) rows of the given voxel keys, in the order of `keys`."""
    k, mu, info = dump
    at = {tuple(int(v) for v in row): i for i, row in enumerate(k)}
    idx = [at[tuple(int(v) for v in row)] for row in keys]
    return mu[idx], info[idx]


def test_incremental_ndt_keeps_its_voxels_when_it_grows(api):
    opts = api.ndt_opts(method=2)  # incremental; the capacity stays at its default, so nothing is evicted
    assert opts.voxel_size == 1.0 and opts.capacity > 3 * 5000
    c1, v1 = _voxel_cloud(0, 55, 55, 1)        # 3 025 voxels: inside the 4 096-slot floor
    c2, v2 = _voxel_cloud(100, 55, 55, 2)      # 3 025 more, elsewhere: across it
    c3, v3 = _voxel_cloud(300, 100, 50, 3)     # 20 000 points: across the 16 384-point floor
    assert v1 < 4096 < v1 + v2 and len(c1) < 16384 and len(c2) < 16384 < len(c3)
    ctx = api.Context(0)
    ctx.ndt_set_target(c1, opts)
    first = ctx.ndt_dump()
    assert len(first[0]) == v1
    keys1 = first[0].copy()
    mu1, info1 = _rows_of(first, keys1)
    total = v1
    for cloud, v in ((c2, v2), (c3, v3)):
        ctx.ndt_set_target(cloud, opts)
        total += v
        dump = ctx.ndt_dump()
        assert len(dump[0]) == total == ctx.ndt_target_info()["num_voxels"]
        mu, info = _rows_of(dump, keys1)
        assert _same(mu, mu1) and _same(info, info1)
    ctx.close()
