"""locgpu_batch_preprocess (RemoveNanPoint → VoxelFilter::Filter on every scan of a batch in one pass), locgpu_batch_upload_clouds and
locgpu_batch_download_scan on the GPU.

Every expected result is built two ways and compared with np.array_equal (points, counts, order, status):
  (a) on the CPU: locref.voxel_grid(finite rows of the scan, dense, leaf, SORT_STABLE)[:, :3];
  (b) on the GPU from the single-cloud entry points: Cloud.upload → remove_nan → voxel_filter → download, per scan.
Shapes are the smallest at which the kernels of csrc/batch_filters.hip can go wrong, not the workload."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# csrc/batch_filters.hip
BLOCK = 256                 # kBF: threads per block of every kernel
BOX_TILE = 1024             # kBoxTile: points a block of the bounding-box pass takes per trip (4 loads in flight per thread)
BOX_BLOCKS_MAX = 64         # kBoxBlocksMax: partial boxes per scan; BOX_TILE * BOX_BLOCKS_MAX points = one trip of a full-width box pass
INVALID = -1
_POOL_CACHE = {}  # expected results of the seven clouds test_scan_bits_of_the_key builds its batches from: computed once


def _cloud(n, seed, scale=10.0, offset=0.0):
    if n == 0:
        return _cloud(1, seed)[:0]  # an empty scan with the row stride of the others
    rng = np.random.default_rng(seed)
    c = (rng.normal(size=(n, 4)) * scale + offset).astype(np.float32)
    c[:, 3] = rng.uniform(0, 255, n).astype(np.float32)  # a batch may carry anything in its fourth lane; the result's is 0
    return c


def _finite_rows(s):
    return s[np.isfinite(s[:, :3]).all(axis=1)]


def _expected(api, ctx, locref, scan, leaf):
    """(points [m, 3], status) of one scan, asserted equal between the CPU oracle (a) and the single-cloud GPU composition (b)."""
    fin = np.ascontiguousarray(_finite_rows(scan))
    a, info = locref.voxel_grid(fin, True, leaf, order=locref.SORT_STABLE, with_info=True)
    c = api.Cloud(ctx, scan, is_dense=False)
    f, passthrough = c.remove_nan().voxel_filter(leaf, with_passthrough=True)
    b = f.download()
    assert np.array_equal(a[:, :3].view(np.uint32), b[:, :3].view(np.uint32)), "oracle and single-cloud filter disagree"
    assert passthrough == (info["status"] == 1)
    return np.ascontiguousarray(a[:, :3]), info["status"]


def _check(api, ctx, locref, scans, leaf, max_points=None, in_place=False, dst_points=None, cache=None):
    """Preprocess `scans` as one batch; every scan must equal its expected result. Returns the downloaded scans."""
    n = len(scans)
    mp = max_points or max(1, max(len(s) for s in scans))
    src = ctx.batch_empty(n, mp)
    src.upload_async(scans)
    exp = []
    for i, s in enumerate(scans):
        key = cache[1][i] if cache else None
        if cache and key in cache[0]:
            exp.append(cache[0][key])
            continue
        e = _expected(api, ctx, locref, s, leaf)
        exp.append(e)
        if cache:
            cache[0][key] = e
    dst = src if in_place else ctx.batch_empty(n, dst_points or max(1, max(len(e[0]) for e in exp)))
    counts, status = src.preprocess(leaf, out=None if in_place else dst)
    got = [dst.download_scan(i) for i in range(n)]
    for i in range(n):
        assert counts[i] == len(exp[i][0]) and status[i] == exp[i][1], (i, counts[i], status[i], len(exp[i][0]), exp[i][1])
        assert got[i].shape == (counts[i], 4)
        assert np.array_equal(got[i][:, :3].view(np.uint32), exp[i][0].view(np.uint32)), i
        assert not got[i][:, 3].view(np.uint32).any(), i  # the fourth lane stays +0
    src.close()
    if not in_place:
        dst.close()
    return got, counts, status


def test_ragged_counts_across_every_tile_edge(api, gpu_ctx, locref):
    full = BOX_TILE * BOX_BLOCKS_MAX
    sizes = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, BOX_TILE - 1, BOX_TILE, BOX_TILE + 1, 4 * BOX_TILE - 1, 4 * BOX_TILE, 4 * BOX_TILE + 1,
             full - 1, full, full + 1]  # the last three are each >= four of the largest tile
    scans = [_cloud(n, 100 + i) for i, n in enumerate(sizes)]
    max_points = full + 33
    assert max_points % 64 != 0
    _, counts, status = _check(api, gpu_ctx, locref, scans, 1.0, max_points=max_points)
    assert status[0] == 2 and counts[0] == 0 and (status[1:] == 0).all()
    assert counts[-1] < sizes[-1]  # the filter merged points


@pytest.mark.parametrize("n_scans", [1, 2, 3, 64, 65, 257])
def test_scan_bits_of_the_key(api, gpu_ctx, locref, n_scans):
    pool = [_cloud(200 + 3 * k, 200 + k, scale=3.0) for k in range(7)]
    which = [0, 0] + [k % 7 for k in range(2, 257)]  # scans 0 and 1 are the same cloud
    scans = [pool[which[i]] for i in range(n_scans)]
    got, _, _ = _check(api, gpu_ctx, locref, scans, 1.0, max_points=227, cache=(_POOL_CACHE, which))
    if n_scans > 1:
        assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))


def test_translated_scans_do_not_merge(api, gpu_ctx, locref):
    base = _cloud(300, 7, scale=2.0)
    base[:, :3] = np.round(base[:, :3] * 64) / 64  # the shifts below are exact: no point changes its voxel by rounding
    scans = []
    for k in range(5):  # whole leaves: every scan has the voxel indices of the first
        s = base.copy()
        s[:, 0] += np.float32(8 * k)
        scans.append(s)
    got, counts, _ = _check(api, gpu_ctx, locref, scans, 1.0)
    assert len(set(counts.tolist())) == 1 and counts[0] > 1
    for k in range(1, 5):
        assert np.abs((got[k][:, 0] - np.float32(8 * k)) - got[0][:, 0]).max() < 1e-4 and np.array_equal(got[k][:, 1:], got[0][:, 1:])


def test_non_finite_points_and_every_status_in_one_batch(api, gpu_ctx, locref):
    leaf = 0.01
    scans = []
    for k in range(3):
        s = _cloud(1500 + 17 * k, 300 + k, scale=0.05)
        s[k::7, k] = np.nan
        s[3::11, (k + 1) % 3] = np.inf
        s[5::13, (k + 2) % 3] = -np.inf
        scans.append(s)
    scans.append(np.full((100, 4), np.nan, np.float32))  # no finite point
    big = _cloud(2000, 310, scale=100.0)                   # leaf too small for its extent: PCL passes the input through
    big[::7, 0] = np.nan
    big[3::11, 2] = np.inf
    big[5::13, 1] = -np.inf
    big[1, 1] = np.float32(-0.0)
    big[2, :3] = np.float32(-0.0)
    assert np.isfinite(big[1, :3]).all() and np.isfinite(big[2, :3]).all()
    scans.insert(2, big)
    # the oracle takes a different branch per scan — the test cannot pass by every scan doing the same thing
    want = [0, 0, 1, 0, 2]
    for s, w in zip(scans, want):
        assert locref.voxel_grid(np.ascontiguousarray(_finite_rows(s)), True, leaf, order=locref.SORT_STABLE, with_info=True)[1]["status"] == w
    got, counts, status = _check(api, gpu_ctx, locref, scans, leaf)
    assert status.tolist() == want and counts[4] == 0
    fin = _finite_rows(big)
    assert np.array_equal(got[2][:, :3].view(np.uint32), fin[:, :3].view(np.uint32))  # bit for bit: the negative zeros too
    assert np.signbit(got[2][:, :3]).any() and (got[2][:, :3].view(np.uint32) == 0x80000000).sum() >= 4


def test_geometry_edges(api, gpu_ctx, locref):
    leaf = 0.5
    rng = np.random.default_rng(5)
    faces = np.zeros((700, 4), np.float32)
    faces[:, :3] = (rng.integers(-9, 10, size=(700, 3)) * leaf).astype(np.float32)  # exactly on voxel faces
    one_voxel = np.zeros((500, 4), np.float32)
    one_voxel[:, :3] = (3.0 + rng.uniform(0.01, 0.49, size=(500, 3))).astype(np.float32)
    scans = [_cloud(900, 50, scale=4.0), -np.abs(_cloud(800, 51, scale=4.0)), faces, one_voxel, _cloud(1, 52), _cloud(333, 53, scale=4.0)]
    scans = [np.ascontiguousarray(s, np.float32) for s in scans]
    _, counts, status = _check(api, gpu_ctx, locref, scans, leaf)
    assert counts[3] == 1 and counts[4] == 1 and (status == 0).all()


def test_in_place_equals_out_of_place_and_runs_repeat(api, gpu_ctx, locref):
    scans = [_cloud(400 + 37 * k, 400 + k, scale=5.0) for k in range(65)]
    scans[40] = _cloud(3000, 499, scale=5.0)
    scans[40][::7, 1] = np.nan
    out1, c1, s1 = _check(api, gpu_ctx, locref, scans, 1.0, max_points=3001)
    out2, c2, s2 = _check(api, gpu_ctx, locref, scans, 1.0, max_points=3001)
    inp, c3, s3 = _check(api, gpu_ctx, locref, scans, 1.0, max_points=3001, in_place=True)
    alone, c4, _ = _check(api, gpu_ctx, locref, [scans[40]], 1.0)
    for i in range(65):
        assert out1[i].tobytes() == out2[i].tobytes() == inp[i].tobytes()
    assert c1.tolist() == c2.tolist() == c3.tolist() and s1.tolist() == s2.tolist() == s3.tolist()
    assert alone[0].tobytes() == out1[40].tobytes() and c4[0] == c1[40]


def test_capacity_failure_leaves_dst_alone(api, gpu_ctx, locref):
    scans = [_cloud(500 + 100 * k, 600 + k, scale=6.0) for k in range(4)]
    exp = [_expected(api, gpu_ctx, locref, s, 1.0)[0] for s in scans]
    need = [len(e) for e in exp]
    src = gpu_ctx.batch(scans)
    dst = gpu_ctx.batch_empty(4, max(need) - 1)
    before = [_cloud(5 + k, 650 + k)[:, :3].copy() for k in range(4)]
    dst.upload_async(before)
    dst.upload_wait()
    with pytest.raises(api.LocGpuError) as e:
        src.preprocess(1.0, out=dst)
    assert e.value.code == INVALID and str(max(need)) in str(e.value)
    assert e.value.counts.tolist() == need
    for k in range(4):
        got = dst.download_scan(k)
        assert np.array_equal(got[:, :3], before[k])
    # the device counts are untouched as well: a pass into a batch that fits, from the refused one as source, sees the old scans
    back = gpu_ctx.batch_empty(4, 16)
    counts, _ = dst.preprocess(1e-3, out=back)
    assert counts.tolist() == [5, 6, 7, 8]
    for b in (src, dst, back):
        b.close()


def test_refusals(api, gpu_ctx):
    scans = [_cloud(50, 700 + k) for k in range(3)]
    plain, other = gpu_ctx.batch(scans), gpu_ctx.batch_empty(3, 50)

    def refused(src, leaf, dst, word):
        with pytest.raises(api.LocGpuError) as e:
            src.preprocess(leaf, out=dst)
        assert e.value.code == INVALID and word in str(e.value), str(e.value)

    sharded = gpu_ctx.batch(scans, first=0, n_total=3)
    refused(sharded, 1.0, other, "sharded")
    refused(plain, 1.0, sharded, "sharded")
    shared = gpu_ctx.batch_shared(scans[0], 3)
    refused(shared, 1.0, other, "shared-source")
    refused(plain, 1.0, shared, "shared-source")
    two = gpu_ctx.batch_empty(2, 50)
    refused(plain, 1.0, two, "numbers of scans")
    ctx2 = api.Context(0)
    foreign = ctx2.batch_empty(3, 50)
    refused(plain, 1.0, foreign, "different contexts")
    foreign.close()
    for leaf in (0.0, -1.0, float("nan"), float("inf")):
        refused(plain, leaf, other, "leaf")
    plain.preprocess(1.0, out=other)
    # begun and not ended (on a context of its own: the shared one keeps whatever target it has)
    busy, idle = ctx2.batch(scans), ctx2.batch_empty(3, 50)
    ctx2.icp_set_target(_cloud(5000, 710)[:, :3].copy())
    poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (3, 1))
    ctx2.icp_align_batch_begin(busy, poses, api.icp_opts(method=api.P2P))
    refused(busy, 1.0, idle, "begun")
    refused(idle, 1.0, busy, "begun")
    refused(busy, 1.0, None, "begun")
    with pytest.raises(api.LocGpuError):
        busy.download_scan(0)
    ctx2.align_batch_end(busy)
    busy.preprocess(1.0, out=idle)
    for b in (plain, other, sharded, shared, two, busy, idle):
        b.close()
    ctx2.close()


def test_downstream_alignment_is_bit_identical(api, locref, synth):
    ctx = api.Context(0)
    leaf = 0.5
    m = synth.make_local_map(20000, 3, half=40.0)
    ctx.icp_set_target(m)
    ctx.ndt_set_target(m)
    _, init = synth.make_pose(3)

    def raw(sub, seed):
        s = synth.make_scan(3, subsample=sub, crop_half=36.0)
        out = np.zeros((len(s), 4), np.float32)
        out[:, :3] = s[:, :3]
        rng = np.random.default_rng(seed)
        out[rng.integers(0, len(s), 40), rng.integers(0, 3, 40)] = np.nan
        out[rng.integers(0, len(s), 5), 0] = np.inf
        return out

    set_a = [raw(3000 + 211 * k, 800 + k) for k in range(5)]
    set_b = [raw(2500 + 173 * k, 900 + k) for k in range(5)]
    poses = np.tile(init, (5, 1))
    opts = api.icp_opts(method=api.P2PLANE)

    def composed(scans):
        clouds = [api.Cloud(ctx, s, is_dense=False).remove_nan().voxel_filter(leaf) for s in scans]
        return clouds, [c.download() for c in clouds]

    def results(batch):
        icp = ctx.icp_align_batch(batch, poses, opts)
        ndt = ctx.ndt_align_batch(batch, poses)
        fit = ctx.icp_fitness_batch(batch, icp[0], max_range=1.0)
        return icp, ndt, fit

    def same(x, y):
        for (px, sx), (py, sy) in zip(x[:2], y[:2]):
            assert px.tobytes() == py.tobytes() and sx == sy
        assert x[2] == y[2]

    clouds_a, host_a = composed(set_a)
    clouds_b, host_b = composed(set_b)
    M = max(len(h) for h in host_a + host_b) + 7
    big = ctx.batch_empty(5, max(len(s) for s in set_a + set_b))
    big.upload_async(set_a)
    dst = ctx.batch_empty(5, M)
    counts, status = big.preprocess(leaf, out=dst)
    assert counts.tolist() == [len(h) for h in host_a] and not status.any()
    resident = ctx.batch_empty(5, M)
    resident.upload_clouds(clouds_a)
    uploaded = ctx.batch_empty(5, M)
    uploaded.upload_async([h[:, :3].copy() for h in host_a])  # the same scans, filtered before the upload and sent through the existing upload path
    for k in range(5):
        assert dst.download_scan(k).tobytes() == resident.download_scan(k).tobytes() == uploaded.download_scan(k).tobytes()
    r_dst = results(dst)
    same(r_dst, results(resident))
    same(r_dst, results(uploaded))
    assert all(s["iterations"] > 0 for s in r_dst[0][1])
    # a captured graph of the preprocessed batch gives the eager result
    ctx.graph_enable(True)
    same(r_dst, results(dst))
    # a second pass into the same dst (its graph is still there) = a fresh dst: no stale counts, graphs or work-list counters
    big.upload_async(set_b)
    big.preprocess(leaf, out=dst)
    r_again = results(dst)
    ctx.graph_enable(False)
    fresh = ctx.batch_empty(5, M)
    big.preprocess(leaf, out=fresh)
    same(r_again, results(fresh))
    for k in range(5):
        assert np.array_equal(dst.download_scan(k)[:, :3], host_b[k][:, :3])
    assert any(len(a) != len(b) for a, b in zip(host_a, host_b))
    for b in (big, dst, resident, uploaded, fresh):
        b.close()
    for c in clouds_a + clouds_b:
        c.close()
    ctx.close()


def test_upload_clouds_and_download_scan(api, gpu_ctx):
    ctx2 = api.Context(0)
    sizes = [0, 1, 65, 1025, 300]
    host = [_cloud(n, 1000 + i) for i, n in enumerate(sizes)]
    clouds = [api.Cloud(ctx2 if i == 3 else gpu_ctx, h) for i, h in enumerate(host)]  # one cloud of another context on the GPU
    b = gpu_ctx.batch_empty(5, 1027)
    b.upload_async([_cloud(1027, 1100 + i) for i in range(5)])  # replaced below, counts included
    b.upload_clouds(clouds)
    L = api.lib()
    for i, h in enumerate(host):
        got = b.download_scan(i)
        assert got.shape == (sizes[i], 4) and np.array_equal(got[:, :3].view(np.uint32), h[:, :3].view(np.uint32)) and not got[:, 3].view(np.uint32).any()
        n = ctypes.c_size_t(99)
        assert L.locgpu_batch_download_scan(b._h, i, None, 0, 12, ctypes.byref(n)) == 0 and n.value == sizes[i]  # count only
    # x, y, z at a 12-byte stride; capacity and index are checked
    out = np.zeros((1025, 3), np.float32)
    n = ctypes.c_size_t(0)
    assert L.locgpu_batch_download_scan(b._h, 3, out.ctypes.data, 1025, 12, ctypes.byref(n)) == 0 and np.array_equal(out, host[3][:, :3])
    assert L.locgpu_batch_download_scan(b._h, 3, out.ctypes.data, 1024, 12, ctypes.byref(n)) == INVALID
    assert L.locgpu_batch_download_scan(b._h, 5, out.ctypes.data, 1025, 12, ctypes.byref(n)) == INVALID
    assert L.locgpu_batch_download_scan(b._h, -1, out.ctypes.data, 1025, 12, ctypes.byref(n)) == INVALID
    # the device counts follow: a pass over the batch sees the clouds' sizes
    counts, status = b.preprocess(1e-4)
    assert counts.tolist() == sizes
    # refusals: a cloud larger than the batch's capacity, the wrong number of clouds
    small = gpu_ctx.batch_empty(5, 1024)
    with pytest.raises(api.LocGpuError) as e:
        small.upload_clouds(clouds)
    assert e.value.code == INVALID
    with pytest.raises(api.LocGpuError):
        b.upload_clouds(clouds[:4])
    shared = gpu_ctx.batch_shared(host[2], 5)
    with pytest.raises(api.LocGpuError):
        shared.upload_clouds(clouds)
    for x in (b, small, shared):
        x.close()
    for c in clouds:
        c.close()
    ctx2.close()
