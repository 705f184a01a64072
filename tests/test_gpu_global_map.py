"""locgpu_clouds_merge, locgpu_batch_merge and locgpu_batch_export_cloud on the GPU (csrc/cloud_merge.hip; Lio::GetGlobalMap,
lio.cpp:550-614).

The reference is the CPU oracle composition of tests/global_map_ref.py (transform_cloud_f64 per cloud → concatenate → voxel_grid);
every comparison is byte for byte: points with the intensity lane, count, is_dense, passthrough. The library's own per-cloud
composition (Cloud.transform / append / voxel_filter) is compared as well. Shapes are the smallest at which the transform-and-join
launch can go wrong (tests/global_map_ref.py says which), not the workload."""
import ctypes

import numpy as np
import pytest

import global_map_ref as gm

pytestmark = pytest.mark.gpu

INVALID = -1
_REF = {}  # oracle results, computed once per (layout, leaf, posed)


def _world(layout):
    key = ("world", layout)
    if key not in _REF:
        counts = gm.LAYOUTS[layout]
        clouds, dense = gm.make_clouds(counts, seed=5 + len(counts))
        _REF[key] = (clouds, dense, gm.make_poses(len(counts)))
    return _REF[key]


def _reference(locref, layout, leaf, posed):
    key = (layout, leaf, posed)
    if key not in _REF:
        clouds, dense, poses = _world(layout)
        _REF[key] = gm.reference(locref, clouds, dense, poses if posed else None, leaf)
    return _REF[key]


def _upload(api, ctx, clouds, dense):
    return [api.Cloud(ctx, c, is_dense=d) for c, d in zip(clouds, dense)]


def _state(cloud):
    n, d = cloud.info
    return cloud.download().tobytes(), n, d


def _assert_is(cloud, passthrough, want, what=""):
    pts, dense, pt = want
    got = cloud.download()
    assert got.shape == pts.shape, (what, got.shape, pts.shape)
    assert np.array_equal(gm.bits(got), gm.bits(pts)), what
    assert cloud.is_dense == dense and passthrough == pt, (what, cloud.is_dense, dense, passthrough, pt)


def _composed(api, ctx, clouds, poses, leaf):
    """GetGlobalMap through the single-cloud entry points: what locgpu_clouds_merge replaces."""
    acc = api.Cloud(ctx)
    for k, c in enumerate(clouds):
        acc.append(c.transform(poses[k]) if poses is not None else c)
    if leaf == 0:
        return acc, False
    return acc.voxel_filter(leaf, with_passthrough=True)


@pytest.mark.parametrize("posed", [True, False])
@pytest.mark.parametrize("layout", sorted(gm.LAYOUTS))
def test_equals_the_oracle_and_the_per_cloud_composition(api, gpu_ctx, locref, layout, posed):
    host, dense, poses = _world(layout)
    clouds = _upload(api, gpu_ctx, host, dense)
    p = poses if posed else None
    for leaf in gm.LEAVES:
        out, pt = gpu_ctx.clouds_merge(clouds, p, leaf, with_passthrough=True)
        want = _reference(locref, layout, leaf, posed)
        _assert_is(out, pt, want, (layout, leaf, posed))
        comp, cpt = _composed(api, gpu_ctx, clouds, p, leaf)
        assert _state(comp) == _state(out) and cpt == pt, (layout, leaf, posed)
    # the cases take the branches they are there for
    assert _reference(locref, layout, 1e-4, posed)[2] and not _reference(locref, layout, 2.0, posed)[2]
    assert len(_reference(locref, layout, 2.0, posed)[0]) < len(_reference(locref, layout, 0.5, posed)[0]) < sum(gm.LAYOUTS[layout])
    # the inputs are as they were
    for c, h, d in zip(clouds, host, dense):
        assert c.download().tobytes() == h.tobytes() and c.is_dense == d


def test_join_order_is_the_list_order(api, gpu_ctx, locref):
    host, dense = gm.make_clouds([1000, 700], seed=21)
    poses = gm.make_poses(2, seed=22)
    poses[:, 6] *= 0.05  # both clouds stay at one height: they share their voxels
    assert gm.shared_voxels(locref, host, dense, poses, 2.0)[0] > 50
    a, b = _upload(api, gpu_ctx, host, dense)
    ab, _ = gpu_ctx.clouds_merge([a, b], poses, 2.0, with_passthrough=True)
    ba, _ = gpu_ctx.clouds_merge([b, a], poses[::-1], 2.0, with_passthrough=True)
    want_ab = gm.reference(locref, host, dense, poses, 2.0)
    want_ba = gm.reference(locref, host[::-1], dense[::-1], poses[::-1], 2.0)
    assert not np.array_equal(gm.bits(want_ab[0]), gm.bits(want_ba[0]))  # the order shows in the reference
    _assert_is(ab, False, want_ab, "[A, B]")
    _assert_is(ba, False, want_ba, "[B, A]")


def test_runs_repeat_and_scratch_growth_changes_nothing(api, locref):
    ctx = api.Context(0)  # its scratch starts empty
    host, dense, poses = _world("straddle")
    clouds = _upload(api, ctx, host, dense)
    first = _state(ctx.clouds_merge(clouds, poses, 0.5))
    assert _state(ctx.clouds_merge(clouds, poses, 0.5)) == first
    big_host, big_dense = gm.make_clouds([60000, 0, 300], seed=31)
    big_poses = gm.make_poses(3, seed=32)
    big = _upload(api, ctx, big_host, big_dense)
    out, pt = ctx.clouds_merge(big, big_poses, 0.5, with_passthrough=True)
    _assert_is(out, pt, gm.reference(locref, big_host, big_dense, big_poses, 0.5), "60 000 points")
    assert _state(ctx.clouds_merge(clouds, poses, 0.5)) == first
    # into a cloud that is reused as the output: the same bytes
    again = ctx.clouds_merge(clouds, poses, 0.5, out=out)
    assert again is out and _state(out) == first
    ctx.close()


def test_clouds_of_a_second_context_are_accepted(api, gpu_ctx, locref):
    ctx2 = api.Context(0)
    host, dense, poses = _world("empty_pair")
    clouds = [api.Cloud(ctx2 if k % 2 == 0 else gpu_ctx, c, is_dense=d) for k, (c, d) in enumerate(zip(host, dense))]
    for leaf in (0.0, 0.5):
        out, pt = gpu_ctx.clouds_merge(clouds, poses, leaf, with_passthrough=True)
        _assert_is(out, pt, _reference(locref, "empty_pair", leaf, True), leaf)
    for c in clouds:
        c.close()
    ctx2.close()


def test_refusals_leave_out_alone(api, gpu_ctx):
    L = api.lib()
    host, dense = gm.make_clouds([40, 600], seed=41)
    a, b = _upload(api, gpu_ctx, host, dense)
    keep = np.arange(20, dtype=np.float32).reshape(5, 4)
    out = api.Cloud(gpu_ctx, keep, is_dense=False)
    before = _state(out)
    assert before[1] == 5 and not before[2]
    ctx2 = api.Context(0)
    foreign_out = api.Cloud(ctx2, keep, is_dense=False)
    h = gpu_ctx._h

    def arr(*cs):
        return (ctypes.c_void_p * len(cs))(*[c._h if c is not None else None for c in cs])

    def refused(rc, word, target=out, was=before):
        assert rc == INVALID
        text = L.locgpu_last_error(h).decode()
        assert "clouds_merge" in text and word in text, text
        assert _state(target) == was

    pt = ctypes.c_int(7)
    ref = ctypes.byref(pt)
    refused(L.locgpu_clouds_merge(h, None, None, 1, 0.5, out._h, ref), "NULL")
    rc = L.locgpu_clouds_merge(h, arr(a, b), None, 2, 0.5, None, ref)
    refused(rc, "NULL")
    refused(L.locgpu_clouds_merge(h, arr(a, None), None, 2, 0.5, out._h, ref), "NULL cloud 1")
    for n in (0, -1):
        refused(L.locgpu_clouds_merge(h, arr(a, b), None, n, 0.5, out._h, ref), "n >= 1")
    for leaf in (-0.5, float("nan"), float("inf"), float("-inf")):
        refused(L.locgpu_clouds_merge(h, arr(a, b), None, 2, leaf, out._h, ref), "leaf")
    refused(L.locgpu_clouds_merge(h, arr(a, out, b), None, 3, 0.5, out._h, ref), "among the inputs")
    refused(L.locgpu_clouds_merge(h, arr(a, b), None, 2, 0.5, foreign_out._h, ref), "another context", foreign_out, before)
    if api.device_count() > 1:
        ctx_far = api.Context(1)
        far = api.Cloud(ctx_far, host[0])
        refused(L.locgpu_clouds_merge(h, arr(a, far), None, 2, 0.5, out._h, ref), "another GPU")
        far.close()
        ctx_far.close()
    # a cloud's limit, 0x7FFFFF00 points in total: one 2^20-point cloud listed 2048 times (checked before any device is touched)
    million = api.Cloud(gpu_ctx, np.zeros((1 << 20, 4), np.float32))
    refused(L.locgpu_clouds_merge(h, arr(*([million] * 2048)), None, 2048, 0.5, out._h, ref), "2^31")
    assert pt.value == 7
    # the same handles are fine once the arguments are
    assert L.locgpu_clouds_merge(h, arr(a, b), None, 2, 0.5, out._h, ref) == 0 and pt.value == 0 and _state(out) != before
    for c in (a, b, out, foreign_out, million):
        c.close()
    ctx2.close()


@pytest.fixture(scope="module")
def batch_world(synth):
    m = synth.make_local_map(20000, 3, half=40.0)
    s = np.ascontiguousarray(synth.make_scan(3, subsample=3000, crop_half=36.0)[:, :3], dtype=np.float32)
    _, init = synth.make_pose(3)
    return m, s, init


def _xyz0(scan):
    out = np.zeros((len(scan), 4), np.float32)
    out[:, :3] = scan[:, :3]
    return out


def test_batch_merge(api, locref, batch_world):
    m, s, init = batch_world
    ctx = api.Context(0)
    ctx.icp_set_target(m)
    max_n = 700
    scans = [s[:0], s[:5], s[5:261], s[261:261 + max_n].copy(), s[-1:]]
    assert [len(x) for x in scans] == [0, 5, 256, max_n, 1]
    scans[3][11, 2] = np.nan
    scans[3][500, 0] = np.inf
    b = ctx.batch(scans)
    poses = gm.make_poses(5, seed=51)
    rounds = []

    def check(tag):
        held = [b.download_scan(k) for k in range(5)]
        exported = [b.export_cloud(k) for k in range(5)]
        for k in range(5):
            assert exported[k].download().tobytes() == _xyz0(held[k]).tobytes() and not exported[k].is_dense, (tag, k)
        host = [_xyz0(x) for x in held]
        for leaf in (0.0, 0.5, 1e-4):
            for use in (None, [0, 1, 0, 1, 0], [0, 0, 0, 0, 0]):
                on = [k for k in range(5) if use is None or use[k]]
                out, pt = b.merge(poses, leaf, use=use, with_passthrough=True)
                if on:
                    want, wpt = ctx.clouds_merge([exported[k] for k in on], poses[on], leaf, with_passthrough=True)
                    assert _state(out) == _state(want) and pt == wpt, (tag, leaf, use)
                    _assert_is(out, pt, gm.reference(locref, [host[k] for k in on], [False] * len(on), poses[on], leaf), (tag, leaf, use))
                else:
                    assert _state(out) == (b"", 0, True) and not pt
        out = b.merge(None, 0.0)  # no poses: the scans' bits, joined
        assert out.download().tobytes() == np.concatenate(host).tobytes() and not out.is_dense
        # the batch is as it was
        for k in range(5):
            assert b.download_scan(k).tobytes() == held[k].tobytes(), (tag, k)
        rounds.append([len(x) for x in held])

    check("raw")
    counts, _ = b.preprocess(0.5)  # in place: NaN removal + voxel filter shrink the counts
    assert counts[3] <= max_n - 2 and counts[0] == 0  # at least the two non-finite points are gone
    # alignment before and after a merge: the same bits
    opts = api.icp_opts(method=api.P2P)
    inits = np.tile(init, (5, 1))
    pose0, st0 = ctx.icp_align_batch(b, inits, opts)
    check("preprocessed")
    pose1, st1 = ctx.icp_align_batch(b, inits, opts)
    assert pose0.tobytes() == pose1.tobytes() and repr(st0) == repr(st1) and st0[3]["iterations"] > 0
    assert rounds[0] != rounds[1]
    b.close()
    ctx.close()


def test_export_cloud_round_trip_and_refusals(api, gpu_ctx, locref, batch_world):
    _, s, _ = batch_world
    sizes = [0, 1, 257, 1000, 64]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    scans = [s[offs[k]:offs[k + 1]] for k in range(5)]
    b = gpu_ctx.batch(scans)
    ctx2 = api.Context(0)
    exported = [b.export_cloud(k, cloud=api.Cloud(ctx2 if k == 3 else gpu_ctx)) for k in range(5)]  # one into a cloud of another context
    assert [len(c) for c in exported] == sizes and not any(c.is_dense for c in exported)
    back = gpu_ctx.batch_empty(5, 1000)
    back.upload_async([s[:1000]] * 5)  # replaced below, counts included
    back.upload_clouds(exported)
    for k in range(5):
        assert back.download_scan(k).tobytes() == b.download_scan(k).tobytes() == _xyz0(scans[k]).tobytes()
    # an exported cloud that is reused shrinks and grows with the scan
    c = b.export_cloud(3)
    assert len(b.export_cloud(1, cloud=c)) == 1 and b.export_cloud(3, cloud=c).download().tobytes() == _xyz0(scans[3]).tobytes()
    # a batch scan as a keyframe: the first keyframe of a local map is the scan under its pose, filtered
    pose = gm.make_poses(1, seed=61)
    sub = api.Submap(gpu_ctx, 2, 0.5)
    sub.add_keyframe(exported[3], pose[0])
    want = gm.reference(locref, [_xyz0(scans[3])], [False], pose, 0.5)
    assert np.array_equal(gm.bits(sub.cloud().download()), gm.bits(want[0]))
    sub.close()

    def refused(fn, word):
        with pytest.raises(api.LocGpuError) as e:
            fn()
        assert e.value.code == INVALID and word in str(e.value), str(e.value)

    keep = api.Cloud(gpu_ctx, _xyz0(scans[4]), is_dense=True)
    before = _state(keep)
    for k in (-1, 5):
        refused(lambda: b.export_cloud(k, cloud=keep), "out of range")
    shared = gpu_ctx.batch_shared(scans[3], 3)
    refused(lambda: shared.export_cloud(0, cloud=keep), "shared-source")
    refused(lambda: shared.merge(None, 0.5, out=keep), "shared-source")
    sharded = gpu_ctx.batch(scans[2:4], first=0, n_total=2)
    refused(lambda: sharded.merge(None, 0.5, out=keep), "sharded")
    for leaf in (-1.0, float("nan"), float("inf")):
        refused(lambda: b.merge(None, leaf, out=keep), "leaf")
    other = api.Cloud(ctx2, _xyz0(scans[4]), is_dense=True)
    refused(lambda: b.merge(None, 0.5, out=other), "another context")
    assert _state(other) == before
    L = api.lib()
    assert L.locgpu_batch_merge(b._h, None, None, 0.5, None, None) == INVALID
    assert L.locgpu_batch_export_cloud(b._h, 0, None) == INVALID
    # begun and not ended, on a context of its own (the shared one keeps whatever target it has)
    busy = ctx2.batch(scans[2:4])
    ctx2.icp_set_target(s)
    ctx2.icp_align_batch_begin(busy, np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (2, 1)), api.icp_opts(method=api.P2P))
    refused(lambda: busy.merge(None, 0.5, out=other), "begun")
    refused(lambda: busy.export_cloud(0, cloud=other), "begun")
    ctx2.align_batch_end(busy)
    assert len(busy.merge(None, 0.0, out=other)) == sizes[2] + sizes[3]
    assert _state(keep) == before
    for x in (b, back, shared, sharded, busy):
        x.close()
    for x in exported + [c, keep, other]:
        x.close()
    ctx2.close()


def test_the_loop_closes(api, locref, batch_world):
    """Align a batch against a prior map, fold it into a map under the poses that came out, make that map the next target."""
    m, s, init = batch_world
    ctx = api.Context(0)
    ctx.icp_set_target(m)
    scans = [s[0:900], s[900:1900], s[1900:3000]]
    b = ctx.batch(scans)
    poses, stats = ctx.icp_align_batch(b, np.tile(init, (3, 1)), api.icp_opts(method=api.P2PLANE))
    assert all(st["iterations"] > 0 for st in stats)
    merged, pt = b.merge(poses, 0.5, with_passthrough=True)
    _assert_is(merged, pt, gm.reference(locref, [_xyz0(x) for x in scans], [False] * 3, poses, 0.5), "merged under the result poses")
    n = len(merged)
    assert 0 < n < 3000
    ctx.icp_set_target_cloud(merged)
    info = ctx.icp_target_info()
    tree = locref.KdTree(merged.download()[:, :3])
    assert (info["num_leaves"], info["num_nodes"], info["depth"]) == (tree.num_leaves, tree.num_nodes, tree.depth)
    assert info["num_leaves"] <= n
    # and the next batch matches against it
    again, stats2 = ctx.icp_align_batch(b, poses, api.icp_opts(method=api.P2P))
    assert np.isfinite(again).all() and all(st["iterations"] > 0 for st in stats2)
    b.close()
    ctx.close()
