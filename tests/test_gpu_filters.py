"""GPU parity of the cloud filters either side of the matcher against oracle/locref_filters.hpp,
through the C ABI (include/locgpu.h: locgpu_cloud_*, locgpu_voxel_filter / crop_box / remove_nan, locgpu_submap_*).

Bars: point sets, counts and ORDER are exact. VoxelGrid centroids are bit-identical to the oracle summing in input order
(SORT_STABLE — the order a stable sort gives, which is what the GPU's radix sort is); against the oracle's std::sort order
(what PCL itself does, unpinned inside a voxel) they agree within float32 summation rounding."""
import numpy as np
import pytest

from conftest import pose_delta

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


def _rand_cloud(n, seed, scale=10.0):
    rng = np.random.default_rng(seed)
    c = (rng.normal(size=(n, 4)) * scale).astype(np.float32)
    c[:, 3] = rng.uniform(0, 255, n).astype(np.float32)
    return c


def _scan_xyzi(synth, scan_id, **kw):
    s = synth.make_scan(scan_id, **kw)
    out = np.zeros((len(s), 4), np.float32)
    out[:, :3] = s[:, :3]
    out[:, 3] = (np.arange(len(s)) % 251).astype(np.float32)
    return out


@pytest.mark.parametrize("leaf", [0.3, 1.0, 2.5])
def test_voxel_filter_bit_exact_vs_stable_oracle(gpu_ctx, locref, leaf):
    c = _rand_cloud(200000, 1)
    got, dense = gpu_ctx.voxel_filter(c, leaf)
    ref = locref.voxel_grid(c, True, leaf, order=locref.SORT_STABLE)
    assert dense and got.shape == ref.shape
    assert np.array_equal(got, ref)
    pcl_like = locref.voxel_grid(c, True, leaf, order=locref.SORT_STD)
    assert np.abs(got - pcl_like).max() <= 256 * EPS * np.abs(c).max()


def test_voxel_filter_on_scan_and_map(gpu_ctx, locref, synth):
    scan = _scan_xyzi(synth, 5)  # full 115 200-pt scan, sensor frame
    for leaf in (0.5, 0.1):
        got, _ = gpu_ctx.voxel_filter(scan, leaf)
        assert np.array_equal(got, locref.voxel_grid(scan, True, leaf, order=locref.SORT_STABLE))
    m = synth.make_map(2_000_000)
    mm = np.zeros((len(m), 4), np.float32)
    mm[:, :3] = m[:, :3]
    got, _ = gpu_ctx.voxel_filter(mm, 0.5)
    ref = locref.voxel_grid(mm, True, 0.5, order=locref.SORT_STABLE)
    assert np.array_equal(got, ref) and len(got) < len(mm)


def test_voxel_filter_non_dense_and_edge_cases(gpu_ctx, locref, api):
    c = _rand_cloud(50000, 2)
    d = c.copy()
    d[::7, 0] = np.nan
    d[3::11, 2] = np.inf
    d[5::13, 1] = -np.inf
    got, dense = gpu_ctx.voxel_filter(d, 1.5, is_dense=False)
    assert dense and np.array_equal(got, locref.voxel_grid(d, False, 1.5, order=locref.SORT_STABLE))
    # not one finite point / empty cloud → empty result
    got, _ = gpu_ctx.voxel_filter(np.full((100, 4), np.nan, np.float32), 1.0, is_dense=False)
    assert len(got) == 0
    got, _ = gpu_ctx.voxel_filter(np.zeros((0, 4), np.float32), 1.0)
    assert len(got) == 0
    # PCL's "leaf size is too small" rule: the input comes back unchanged, flag included
    big = _rand_cloud(5000, 3, scale=100.0)
    got, dense = gpu_ctx.voxel_filter(big, 0.01, is_dense=False)
    assert np.array_equal(got, big) and not dense
    ref, info = locref.voxel_grid(big, False, 0.01, with_info=True)
    assert info["status"] == 1
    # single point, all points in one voxel, negative coordinates
    for cloud, leaf in ((c[:1], 1.0), (np.abs(c[:1000]) % 1.0, 2.0), (-np.abs(c[:1000]), 0.7)):
        cloud = np.ascontiguousarray(cloud, np.float32)
        got, _ = gpu_ctx.voxel_filter(cloud, leaf)
        assert np.array_equal(got, locref.voxel_grid(cloud, True, leaf, order=locref.SORT_STABLE))
    with pytest.raises(api.LocGpuError):
        gpu_ctx.voxel_filter(c, 0.0)
    with pytest.raises(api.LocGpuError):
        gpu_ctx.voxel_filter(c, float("nan"))


def test_crop_box_and_remove_nan_exact(gpu_ctx, locref):
    c = _rand_cloud(300000, 4)
    mn, mx = locref.box_edges([6, 5, 4], [1.25, -0.5, 0.125])
    got, dense = gpu_ctx.crop_box(c, mn, mx)
    assert dense and np.array_equal(got, locref.crop_box(c, True, mn, mx))
    d = c.copy()
    d[::5, 2] = np.nan
    d[1::9, 0] = np.inf
    # dense flag trusted: NaN coordinates pass every comparison and are kept
    got, _ = gpu_ctx.crop_box(d, mn, mx, is_dense=True)
    assert np.array_equal(got, locref.crop_box(d, True, mn, mx), equal_nan=True)
    got, _ = gpu_ctx.crop_box(d, mn, mx, is_dense=False)
    assert np.array_equal(got, locref.crop_box(d, False, mn, mx))
    # bounds are inclusive
    e = np.array([[1, 1, 1, 0], [2, 0, 0, 1], [-2, 0, 0, 2], [2.0001, 0, 0, 3]], np.float32)
    got, _ = gpu_ctx.crop_box(e, [-2, -2, -2], [2, 2, 2])
    assert [int(v) for v in got[:, 3]] == [0, 1, 2]
    # removeNaN: dense clouds pass untouched, others keep the finite points in order
    got, dn = gpu_ctx.remove_nan(d, True)
    assert dn and np.array_equal(got, d, equal_nan=True)
    got, dn = gpu_ctx.remove_nan(d, False)
    assert dn and np.array_equal(got, locref.remove_nan(d, False))
    got, _ = gpu_ctx.crop_box(c, [100, 100, 100], [101, 101, 101])
    assert len(got) == 0


def test_resident_pipeline_matches_host_pipeline(gpu_ctx, locref, synth, api, small_world):
    """Loc::Update's front (loc.cpp:217-224) on a resident cloud: removeNaN → voxel filter → ScanMatch, one upload."""
    scan = _scan_xyzi(synth, 3, crop_half=36.0)
    scan[::97, 1] = np.nan
    raw = api.Cloud(gpu_ctx, scan, is_dense=False)
    assert raw.info == (len(scan), False)
    filt = raw.remove_nan().voxel_filter(0.5)
    ref = locref.voxel_grid(locref.remove_nan(scan, False), True, 0.5, order=locref.SORT_STABLE)
    assert np.array_equal(filt.download(), ref) and filt.is_dense
    # match the filtered scan: resident path == host-pointer path == oracle
    gpu_ctx.icp_set_target(small_world["map"])
    opts = api.icp_opts(api.P2PLANE)
    pose_dev, st_dev = gpu_ctx.icp_align_cloud(filt, small_world["init_pose"], opts)
    pose_host, st_host = gpu_ctx.icp_align(ref, small_world["init_pose"], opts)
    assert np.array_equal(pose_dev, pose_host) and st_dev["iterations"] == st_host["iterations"]
    icp = locref.Icp(method=locref.P2PLANE)
    icp.set_target(small_world["map"])
    res = icp.align(ref, small_world["init_pose"])
    dt, dr = pose_delta(pose_dev, res["pose"])
    assert dt < 1e-8 and dr < 1e-8 and res["iters"] == st_dev["iterations"]
    # NDT on resident clouds: target table built from a resident map
    mapc = np.zeros((len(small_world["map"]), 4), np.float32)
    mapc[:, :3] = small_world["map"][:, :3]
    target = api.Cloud(gpu_ctx, mapc)
    gpu_ctx.ndt_set_target_cloud(target)
    pose_dev, st = gpu_ctx.ndt_align_cloud(filt, small_world["init_pose"])
    gpu_ctx.ndt_set_target(small_world["map"])
    pose_host, st2 = gpu_ctx.ndt_align(ref, small_world["init_pose"])
    assert np.array_equal(pose_dev, pose_host) and st["iterations"] == st2["iterations"]
    # ICP target from a resident cloud == from the host cloud
    gpu_ctx.icp_set_target_cloud(target)
    pose_t, _ = gpu_ctx.icp_align_cloud(filt, small_world["init_pose"], opts)
    gpu_ctx.icp_set_target(small_world["map"])
    pose_h, _ = gpu_ctx.icp_align_cloud(filt, small_world["init_pose"], opts)
    assert np.array_equal(pose_t, pose_h)


def test_cloud_transform_append_copy(gpu_ctx, locref, api):
    c = _rand_cloud(100000, 6, scale=40.0)
    q = np.array([0.05, -0.02, 0.6, 0.8])
    pose = np.concatenate([q / np.linalg.norm(q), [12.5, -40.25, 1.0]])
    a = api.Cloud(gpu_ctx, c)
    t = a.transform(pose)
    assert np.array_equal(t.download(), locref.transform_cloud_f64(pose, c))
    a.transform(pose, out=a)  # in place
    assert np.array_equal(a.download(), locref.transform_cloud_f64(pose, c))
    d = c.copy()
    d[::3, 1] = np.nan
    nd = api.Cloud(gpu_ctx, d, is_dense=False)
    assert np.array_equal(nd.transform(pose).download(), locref.transform_cloud_f64(pose, d, is_dense=False), equal_nan=True)
    b = api.Cloud(gpu_ctx, c[:1000])
    b.append(nd)
    assert len(b) == 1000 + len(d) and not b.is_dense
    assert np.array_equal(b.download(), np.concatenate([c[:1000], d]), equal_nan=True)
    cp = b.copy()
    assert np.array_equal(cp.download(), b.download(), equal_nan=True) and cp.info == b.info
    e = api.Cloud(gpu_ctx)
    assert e.info == (0, True) and len(e.download()) == 0
    e.append(b)
    assert len(e) == len(b)


def test_submap_follows_lio_keyframe_branch(gpu_ctx, locref, synth, api):
    """lio.cpp:268-306 over 6 keyframes with num_kfs = 3: transform, append / rebuild, in-place voxel filter."""
    sub = api.Submap(gpu_ctx, 3, 0.5)
    lm = locref.LocalMap(3, 0.5, order=locref.SORT_STABLE)
    for s in range(6):
        scan = _scan_xyzi(synth, 4 * s, subsample=30000)
        true_pose, _ = synth.make_pose(4 * s)
        sub.add_keyframe(api.Cloud(gpu_ctx, scan), true_pose)
        kf = locref.transform_cloud_f64(true_pose, scan)
        lm.add_keyframe(kf)
        assert np.array_equal(sub.last_keyframe().download(), kf)
        got = sub.cloud().download()
        assert np.array_equal(got, lm.cloud())
        assert sub.info == (min(s + 1, 3), len(got))
    # the local map is a valid matching target: align the next scan against it, resident vs oracle
    gpu_ctx.icp_set_target_cloud(sub.cloud())
    scan = synth.make_scan(21, subsample=10000)
    true_pose, init_pose = synth.make_pose(21)
    opts = api.icp_opts(api.P2PLANE)
    pose, st = gpu_ctx.icp_align(scan, init_pose, opts)
    icp = locref.Icp(method=locref.P2PLANE)
    icp.set_target(lm.cloud()[:, :3])
    res = icp.align(scan, init_pose)
    dt, dr = pose_delta(pose, res["pose"])
    assert dt < 1e-8 and dr < 1e-8 and st["iterations"] == res["iters"]
    # world-frame keyframes (pose = None) take the same path
    sub2 = api.Submap(gpu_ctx, 2, 1.0)
    lm2 = locref.LocalMap(2, 1.0, order=locref.SORT_STABLE)
    for s in range(3):
        kf = _rand_cloud(20000, 40 + s, scale=8.0)
        sub2.add_keyframe(api.Cloud(gpu_ctx, kf))
        lm2.add_keyframe(kf)
        assert np.array_equal(sub2.cloud().download(), lm2.cloud())


def test_filter_error_paths(gpu_ctx, api):
    other = api.Context(0)
    try:
        a = api.Cloud(gpu_ctx, _rand_cloud(10, 1))
        b = api.Cloud(other)
        with pytest.raises(api.LocGpuError):
            a.voxel_filter(1.0, out=b)  # clouds of different contexts
        with pytest.raises(api.LocGpuError):
            other.icp_align_cloud(a, np.array([0, 0, 0, 1, 0, 0, 0.0]), api.icp_opts(api.P2PLANE))
        with pytest.raises(api.LocGpuError):
            gpu_ctx.icp_set_target_cloud(api.Cloud(gpu_ctx))  # empty target
        with pytest.raises(api.LocGpuError):
            api.Submap(gpu_ctx, 0, 0.5)
    finally:
        other.close()


@pytest.mark.parametrize("dense", [1, 0])
def test_cpp_facade_filters(locref, synth, tmp_path, dense):
    """LocUtils::VoxelFilter / BoxFilter / gpu::RemoveNanPoint (loc_lib_amd/host) driven like Loc::Update and ResetLocalMap."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(__file__), "cpp", "facade_filters")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    cloud = _scan_xyzi(synth, 9)
    cloud[::53, 2] = np.nan
    cloud.tofile(tmp_path / "in.bin")
    origin, half, leaf = (3.5, -2.25, 0.5), 20.0, 0.5
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(dense), str(leaf), *[str(v) for v in origin], str(half), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    m_scan, m_box = int(tok[0]), int(tok[1])
    edge = np.array([float(t) for t in tok[2:8]], np.float32)
    scan = np.fromfile(str(tmp_path / "out.scan.bin"), np.float32).reshape(-1, 4)
    box = np.fromfile(str(tmp_path / "out.box.bin"), np.float32).reshape(-1, 4)
    assert len(scan) == m_scan and len(box) == m_box
    mn, mx = locref.box_edges([half] * 3, origin)
    assert np.array_equal(edge[0::2], mn) and np.array_equal(edge[1::2], mx)
    assert np.array_equal(box, locref.crop_box(cloud, bool(dense), mn, mx), equal_nan=True)
    no_nan = locref.remove_nan(cloud, bool(dense))
    if dense:
        # a cloud flagged dense is never tested: the NaNs survive removeNaN and reach VoxelGrid, whose index arithmetic on
        # NaN is undefined in PCL — only the finite voxels are comparable, so just check the call completed
        assert int(tok[8]) == 1
    else:
        want = locref.voxel_grid(no_nan, True, leaf, order=locref.SORT_STABLE)
        assert np.array_equal(scan, want) and int(tok[8]) == 1


def test_golden_filter_fixture_gpu(gpu_ctx, api):
    """Committed golden vectors (tests/golden/make_golden_filters.py, generated with the oracle in the build container)."""
    import os
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "filters_small_scan.npz")))
    g.update(np.load(os.path.join(os.path.dirname(__file__), "golden", "filters_small_maps.npz")))
    scan = g["scan"]
    got, dense = gpu_ctx.remove_nan(scan, False)
    assert dense and np.array_equal(got, g["no_nan"])
    got, _ = gpu_ctx.voxel_filter(g["no_nan"], 0.4)
    assert np.array_equal(got, g["voxel_stable"])
    assert np.abs(got - g["voxel_std"]).max() <= 256 * EPS * np.abs(g["no_nan"]).max()
    got, _ = gpu_ctx.voxel_filter(scan, 0.4, is_dense=False)
    assert np.array_equal(got, g["voxel_nondense_stable"])
    got, _ = gpu_ctx.crop_box(scan, g["box_min"], g["box_max"], is_dense=True)
    assert np.array_equal(got, g["crop_dense"], equal_nan=True)
    got, _ = gpu_ctx.crop_box(scan, g["box_min"], g["box_max"], is_dense=False)
    assert np.array_equal(got, g["crop_nondense"])
    sub = api.Submap(gpu_ctx, 3, 0.6)
    for s in range(5):
        sub.add_keyframe(api.Cloud(gpu_ctx, g["kf_scan_%d" % s]), g["kf_pose_%d" % s])
        if s == 0:
            assert np.array_equal(sub.last_keyframe().download(), g["kf_world_0"])
        assert np.array_equal(sub.cloud().download(), g["local_map_%d" % s])
    edge, surf = api.Cloud(gpu_ctx, g["loam_cloud"]).loam_extract(g["loam_ring"], 16)
    assert np.array_equal(edge.download(), g["loam_edge"]) and np.array_equal(surf.download(), g["loam_surf"])


def test_voxel_filter_of_a_non_dense_cloud_equals_remove_nan_then_filter(gpu_ctx, api, locref):
    """The per-scan path of the front-ends (RemoveNanPoint, then VoxelFilter::Filter; lio.cpp:236) as ONE call: pcl::VoxelGrid skips
    non-finite points of a cloud that is not flagged dense, in getMinMax3D and in its key pass alike, so filtering the raw scan gives
    the same cloud bit for bit — with one host read-back (scan-sized clouds) instead of three. Also the two rare outcomes that are
    now detected after the fact: no finite point at all, and a leaf so small that PCL passes the input through."""
    rng = np.random.default_rng(11)
    pts = rng.uniform(-40, 40, size=(60000, 4)).astype(np.float32)
    bad = rng.choice(len(pts), 900, replace=False)
    pts[bad[:300], 0] = np.nan
    pts[bad[300:600], 2] = np.inf
    pts[bad[600:], 1] = -np.inf
    raw = api.Cloud(gpu_ctx, pts, is_dense=False)
    one = raw.voxel_filter(0.5)
    two = raw.remove_nan().voxel_filter(0.5)
    assert np.array_equal(one.download(), two.download()) and one.is_dense
    want = locref.voxel_grid(locref.remove_nan(pts, False), True, 0.5, order=locref.SORT_STABLE)
    assert np.array_equal(one.download(), want)
    empty = api.Cloud(gpu_ctx, np.full((100, 4), np.nan, np.float32), is_dense=False).voxel_filter(0.5)
    assert len(empty) == 0
    wide = np.zeros((4, 4), np.float32)
    wide[1, :3] = 3.0e5
    wide[2, :3] = -3.0e5
    through = api.Cloud(gpu_ctx, wide, is_dense=True).voxel_filter(0.01)  # 6e7 cells per axis: "leaf size is too small"
    assert np.array_equal(through.download(), wide)

def test_async_target_ingest_equals_the_blocking_one(api, locref, synth, small_world):
    """locgpu_icp_set_target_cloud_async: the host tree build runs on a worker while the caller goes on (here: uploads and filters a
    scan, as Lio::AddCloud would between a keyframe and the next ScanMatch); the first reader of the target completes the ingest.
    Same tree (target_info) and same pose as the blocking call; the next reader always sees the new target; a second SetInputTarget
    supersedes a pending one; target_info alone completes one; a context destroyed with an ingest pending shuts down cleanly."""
    m, s, init = small_world["map"], small_world["scan10k"], small_world["init_pose"]
    opts = api.icp_opts(method=api.P2PLANE)

    def cloud4(a):
        out = np.zeros((len(a), 4), np.float32)
        out[:, :3] = a[:, :3]
        return out

    ctx = api.Context(0)
    try:
        big, small = api.Cloud(ctx, cloud4(m)), api.Cloud(ctx, cloud4(m[::7]))
        ctx.icp_set_target_cloud(big)
        want_info = ctx.icp_target_info()
        want_pose, want_st = ctx.icp_align(s, init, opts)
        ctx.icp_set_target_cloud(small)
        small_info = ctx.icp_target_info()
        small_pose, _ = ctx.icp_align(s, init, opts)
        assert small_info != want_info
        for rep in range(3):
            ctx.icp_set_target_cloud(small)                       # something else in place first
            ctx.icp_set_target_cloud(big, wait=False)             # returns with the build running
            raw = api.Cloud(ctx, cloud4(s))                       # the caller's own work in the meantime
            raw.voxel_filter(0.5)
            pose, st = ctx.icp_align(s, init, opts)               # completes the ingest first
            assert np.array_equal(pose, want_pose) and st["iterations"] == want_st["iterations"]
            assert ctx.icp_target_info() == want_info
        # superseded: async(big) then blocking(small) ⇒ small wins, whenever the worker finishes
        ctx.icp_set_target_cloud(big, wait=False)
        ctx.icp_set_target_cloud(small)
        assert ctx.icp_target_info() == small_info
        assert np.array_equal(ctx.icp_align(s, init, opts)[0], small_pose)
        # target_info alone completes a pending ingest
        ctx.icp_set_target_cloud(big, wait=False)
        assert ctx.icp_target_info() == want_info
        # the host-pointer version: the caller's array may be overwritten as soon as the call returns
        mm = np.ascontiguousarray(m, dtype=np.float32).copy()
        ctx.icp_set_target(mm, wait=False)
        mm[:] = 0.0
        assert ctx.icp_target_info() == want_info
        assert np.array_equal(ctx.icp_align(s, init, opts)[0], want_pose)
        with pytest.raises(api.LocGpuError):
            ctx.icp_set_target(np.zeros((0, 3), np.float32), wait=False)
        ctx.icp_set_target_cloud(small, wait=False)               # left pending: destroy must cope
    finally:
        ctx.close()
