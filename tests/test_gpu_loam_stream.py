"""The LOAM matcher on resident clouds (locgpu_loam_set_target_cloud[_async], locgpu_loam_scan_match_cloud, locgpu_loam_fitness_resident,
locgpu_loam_submap_*): Lio::AddCloud(FullCloudPtr) (lio.cpp:311-410) with AlignWithLocalMap (:475-502) composed without a PCIe hop.
Feature scans are the first 16 rings (28 800 points, ring = index // 1800) of synth.make_scan(i); voxel leaf 0.5 for scans and maps.
The resident calls are held to the host-pointer calls bit for bit, the streaming loop to the oracle composition of tests/loam_ref.py."""
import numpy as np
import pytest

import loam_ref
from conftest import pose_delta

pytestmark = pytest.mark.gpu

N_PTS, NUM_SCAN, RING_LEN = 28800, 16, 1800
LEAF = 0.5
SCAN_IDS = (0, 1, 2, 3, 4, 5, 6)  # the oracle alone aligns 1..6 with status 0 (checked on the CPU before the GPU saw them)
KEYFRAMES = (0, 2, 4, 6)
NUM_KFS = 2
POSE_TOL = 1e-8  # metres and radians: the bar of test_streaming_loop_matches_oracle (tests/test_gpu_configs.py) for the same kind of loop


def raw_scan(synth, i):
    """(cloud [28800, 4] with an intensity that tells points apart, ring [28800])"""
    s = synth.make_scan(i)[:N_PTS]
    assert len(s) == N_PTS
    c = np.zeros((N_PTS, 4), np.float32)
    c[:, :3] = s[:, :3]
    c[:, 3] = (np.arange(N_PTS) % 256).astype(np.float32)
    return c, (np.arange(N_PTS) // RING_LEN).astype(np.uint8)


def features(locref, synth, i):
    """The picker's UNFILTERED (edge, surf) of scan i on the CPU."""
    c, ring = raw_scan(synth, i)
    return locref.loam_extract(c, ring, NUM_SCAN, order=locref.SORT_STABLE)


class CpuLio:
    """The CPU side of Lio::AddCloud(FullCloudPtr)'s map keeping (lio.cpp:331-409), written out: locref.LocalMap always filters, and
    the first keyframe must not be."""

    def __init__(self, locref, leaf=LEAF, num_kfs=NUM_KFS):
        self.locref, self.leaf, self.num_kfs = locref, leaf, num_kfs
        self.kf_e, self.kf_s = [], []
        self.map_e = self.map_s = self.oracle = None

    def _filter(self, c):
        return self.locref.voxel_grid(c, True, self.leaf, order=self.locref.SORT_STABLE)

    def filter_scan(self, e, s):  # AlignWithLocalMap filters both in place (:485-486)
        return self._filter(e), self._filter(s)

    def add_keyframe(self, e, s, pose):
        ke, ks = self.locref.transform_cloud_f64(pose, e), self.locref.transform_cloud_f64(pose, s)  # :343-344, :379-380
        first = not self.kf_e
        self.kf_e.append(ke)
        self.kf_s.append(ks)
        if first:
            self.map_e, self.map_s = ke, ks  # :348-349 the first keyframe IS both maps, unfiltered (the filter at :338-339 saw empty maps)
        else:
            if len(self.kf_e) > self.num_kfs:  # :385-398 drop the oldest, rebuild
                self.kf_e.pop(0)
                self.kf_s.pop(0)
                self.map_e, self.map_s = np.vstack(self.kf_e), np.vstack(self.kf_s)
            else:  # :399-403
                self.map_e, self.map_s = np.vstack([self.map_e, ke]), np.vstack([self.map_s, ks])
            self.map_e, self.map_s = self._filter(self.map_e), self._filter(self.map_s)  # :405-406
        self.oracle = loam_ref.LoamOracle(self.locref, self.map_e[:, :3], self.map_s[:, :3])  # :346, :408


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32)


@pytest.fixture(scope="module")
def world(locref, synth):
    """CPU data computed once and never modified: the first keyframe's maps (scan 0 at its true pose, unfiltered), the maps after a
    second keyframe (scan 1's filtered features at its true pose), and the filtered feature scans 1 and 2 with their initial poses."""
    lio = CpuLio(locref)
    e0, s0 = features(locref, synth, 0)
    lio.add_keyframe(e0, s0, synth.make_pose(0)[0])
    w = dict(edge_map=lio.map_e, surf_map=lio.map_s)
    for i in (1, 2):
        w["edge%d" % i], w["surf%d" % i] = lio.filter_scan(*features(locref, synth, i))
        w["init%d" % i] = np.array(synth.make_pose(i)[1], dtype=np.float64)
    lio.add_keyframe(w["edge1"], w["surf1"], synth.make_pose(1)[0])
    w["edge_map2"], w["surf_map2"] = lio.map_e, lio.map_s
    assert len(w["edge1"]) > 100 and len(w["surf1"]) > 1000
    return w


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


def _handle(api, world, which):
    h = api.Loam(api.loam_opts(use_edge_points=int(which != "surf_only"), use_surf_points=int(which != "edge_only")))
    h.set_target(None if which == "surf_only" else world["edge_map"], None if which == "edge_only" else world["surf_map"])
    return h


@pytest.mark.parametrize("which", ["both", "surf_only", "edge_only"])
def test_resident_equals_host_pointer_bit_for_bit(api, ctx, world, which):
    """surf_only still hands the edge cloud (a switched-off class's points join the output); edge_only hands no surface cloud. In
    `both` the edge cloud is flagged not dense."""
    e, s, init = world["edge1"], world["surf1"], world["init1"]
    e_in, s_in = e, (None if which == "edge_only" else s)
    e_dense = which != "both"
    h = _handle(api, world, which)
    try:
        pose_h, st_h, cloud_h = h.scan_match(e_in, s_in, init)
        ec = api.Cloud(ctx, e_in, is_dense=e_dense)
        sc = api.Cloud(ctx, s_in) if s_in is not None else None
        out = api.Cloud(ctx)
        pose_r, st_r = h.scan_match_cloud(ec, sc, init, out=out)
        print(which, "host", st_h, "resident", st_r)
        assert st_h["status"] == 0 and st_h["iterations"] > 1
        assert np.array_equal(_bits(pose_r), _bits(pose_h)) and st_r == st_h
        got = out.download()
        inputs = [e_in] + ([s_in] if s_in is not None else [])
        assert len(got) == sum(len(c) for c in inputs) == len(cloud_h)
        assert np.array_equal(_bits(got[:, :3]), _bits(cloud_h))
        assert np.array_equal(_bits(got[:, 3]), _bits(np.concatenate([c[:, 3] for c in inputs])))
        assert out.is_dense == e_dense
        # out must be distinct from the inputs
        with pytest.raises(api.LocGpuError) as err:
            h.scan_match_cloud(ec, sc, init, out=ec)
        assert err.value.code == -1
    finally:
        h.close()


def test_a_failing_class_leaves_pose_and_out_untouched_in_both_paths(api, ctx, world):
    e, s, init = world["edge1"][:5], world["surf1"], world["init1"]
    sentinel = np.array([0.5, -0.5, 0.5, -0.5, 11.0, 12.0, 13.0])
    h = _handle(api, world, "both")
    try:
        host_out = np.full((len(e) + len(s), 3), 7.5, np.float32)
        pose_h, st_h, _ = h.scan_match(e, s, init, result_pose=sentinel, out_cloud=host_out)
        before = np.full((9, 4), 2.5, np.float32)
        out = api.Cloud(ctx, before, is_dense=False)
        pose_r, st_r = h.scan_match_cloud(api.Cloud(ctx, e), api.Cloud(ctx, s), init, result_pose=sentinel, out=out)
        assert st_h["status"] == st_r["status"] == 4 and st_r == st_h, (st_h, st_r)
        assert np.array_equal(pose_h, sentinel) and np.array_equal(pose_r, sentinel) and (host_out == 7.5).all()
        assert np.array_equal(out.download(), before) and not out.is_dense
    finally:
        h.close()


def test_async_target_equals_blocking_target(api, ctx, world):
    maps = [api.Cloud(ctx, world[k]) for k in ("edge_map", "surf_map", "edge_map2", "surf_map2")]
    scans = [(api.Cloud(ctx, world["edge%d" % i]), api.Cloud(ctx, world["surf%d" % i]), world["init%d" % i]) for i in (1, 2)]
    poses = {}
    for wait in (True, False):
        h = api.Loam()
        try:
            h.set_target_cloud(maps[0], maps[1], wait=wait)
            p1, st1 = h.scan_match_cloud(*scans[0])
            old2, _ = h.scan_match_cloud(*scans[1])  # scan 2 against the FIRST maps
            h.set_target_cloud(maps[2], maps[3], wait=wait)
            p2, st2 = h.scan_match_cloud(*scans[1])  # ... and against the new ones: the pending ingest ends inside this call
            assert st1["status"] == st2["status"] == 0
            assert not np.array_equal(p2, old2)
            poses[wait] = (p1, st1, p2, st2)
        finally:
            h.close()
    for a, b in zip(poses[True], poses[False]):
        assert np.array_equal(_bits(a), _bits(b)) if isinstance(a, np.ndarray) else a == b


def test_streaming_loop_matches_oracle(api, ctx, locref, synth):
    """Scan ids 0..6, keyframes on 0, 2, 4 and 6, two keyframes in the maps (the fourth keyframe drops the oldest and rebuilds). The
    oracle alone — the CPU side below with its own poses as keyframe poses — aligns every one of scans 1..6 with status 0 at leaf 0.5."""
    h = api.Loam()
    try:
        sub = api.LoamSubmap(ctx, NUM_KFS, LEAF)
        lio = CpuLio(locref)
        raw = api.Cloud(ctx)
        for i in SCAN_IDS:
            c, ring = raw_scan(synth, i)
            truth, init = synth.make_pose(i)
            raw.upload(c)  # the scan crosses PCIe once
            edge, surf = raw.loam_extract(ring, NUM_SCAN)
            e_ref, s_ref = locref.loam_extract(c, ring, NUM_SCAN, order=locref.SORT_STABLE)
            if i == SCAN_IDS[0]:
                pose = np.array(truth, dtype=np.float64)  # `pose = last_kf_pose_` (:336): no match, the features stay unfiltered
            else:
                edge.voxel_filter(LEAF, out=edge)
                surf.voxel_filter(LEAF, out=surf)
                e_ref, s_ref = lio.filter_scan(e_ref, s_ref)
                pose, st = h.scan_match_cloud(edge, surf, init)
                want = lio.oracle.scan_match(e_ref[:, :3], s_ref[:, :3], init)
                dt, dr = pose_delta(pose, want["pose"])
                print("scan %d: %d edge, %d surf, iterations %d (oracle %d), status %d (oracle %d), dt %.3e m, dr %.3e rad" %
                      (i, len(e_ref), len(s_ref), st["iterations"], want["iterations"], st["status"], want["status"], dt, dr))
                assert want["status"] == 0, (i, want)  # the condition of this test: no scan skipped, every oracle alignment good
                assert st["status"] == want["status"] and st["iterations"] == want["iterations"], (i, st, want)
                assert dt < POSE_TOL and dr < POSE_TOL, (i, dt, dr)
            if i in KEYFRAMES:
                assert np.array_equal(_bits(edge.download()), _bits(e_ref)) and np.array_equal(_bits(surf.download()), _bits(s_ref)), i
                sub.add_keyframe(edge, surf, pose)  # the unfiltered features first, the filtered ones from then on
                h.set_target_cloud(*sub.clouds())
                lio.add_keyframe(e_ref, s_ref, pose)
                em, sm = sub.clouds()
                assert np.array_equal(_bits(em.download()), _bits(lio.map_e)) and np.array_equal(_bits(sm.download()), _bits(lio.map_s)), i
                assert sub.info == (min(len(lio.kf_e), NUM_KFS), len(lio.map_e), len(lio.map_s))
        assert sub.info[0] == NUM_KFS and len(lio.kf_e) == NUM_KFS
        sub.close()
    finally:
        h.close()


def test_fitness_resident_equals_icp_fitness_of_each_class(api, ctx, world):
    e, s, init = world["edge1"], world["surf1"], world["init1"]
    nothing = dict(score=np.inf, inliers=0, finite_points=0)
    h = _handle(api, world, "both")
    plain = api.Context(0)
    try:
        with pytest.raises(api.LocGpuError) as err:
            h.fitness_resident(init)
        assert err.value.code == -1  # LOCGPU_ERR_INVALID: nothing is resident yet
        ec, sc = api.Cloud(ctx, e), api.Cloud(ctx, s)
        pose, st = h.scan_match_cloud(ec, sc, init)
        got = h.fitness_resident(pose, 1.0)
        plain.icp_set_target(world["surf_map"])
        want_s = plain.icp_fitness(s, pose, 1.0)
        plain.icp_set_target(world["edge_map"])
        want_e = plain.icp_fitness(e, pose, 1.0)
        print("surface", got[0], "edge", got[1])
        assert got[0] == want_s and got[1] == want_e
        assert got[0]["inliers"] > 0 and got[1]["inliers"] > 0
        # the host-pointer call leaves its own copies: the same scores
        h.scan_match(e, s, init)
        assert h.fitness_resident(pose, 1.0) == got
        # a batched call leaves nothing of a single scan
        h.align_batch([e, e], [s, s], np.array([init, init]))
        with pytest.raises(api.LocGpuError) as err:
            h.fitness_resident(pose)
        assert err.value.code == -1
    finally:
        h.close()
        plain.close()
    h = _handle(api, world, "surf_only")
    try:
        pose, st = h.scan_match_cloud(None, api.Cloud(ctx, s), init)
        got = h.fitness_resident(pose, 1.0)
        assert got[1] == nothing and got[0]["inliers"] > 0
    finally:
        h.close()


def test_scans_of_another_context_match_like_the_handles_own(api, ctx, world, synth):
    """Upload, extraction and filter on a separate front-end context, the match through the handle with maps and output on `ctx`: the
    handle's stream has to go behind the front-end's (cloud_input_ready). Equal to the run with everything on one context."""
    c, ring = raw_scan(synth, 1)
    init = world["init1"]
    h = api.Loam()
    front = api.Context(0)
    try:
        h.set_target_cloud(api.Cloud(ctx, world["edge_map"]), api.Cloud(ctx, world["surf_map"]))
        runs = []
        for owner in (ctx, front):
            edge, surf = api.Cloud(owner, c).loam_extract(ring, NUM_SCAN)
            edge.voxel_filter(LEAF, out=edge)
            surf.voxel_filter(LEAF, out=surf)
            out = api.Cloud(ctx)
            pose, st = h.scan_match_cloud(edge, surf, init, out=out)
            runs.append((pose, st, out.download(), h.fitness_resident(pose)))
            edge.close()
            surf.close()
        (p0, st0, out0, fit0), (p1, st1, out1, fit1) = runs
        assert st0["status"] == 0 and np.array_equal(_bits(p0), _bits(p1)) and st0 == st1 and fit0 == fit1
        assert len(out0) == len(world["edge1"]) + len(world["surf1"]) and np.array_equal(_bits(out0), _bits(out1))
    finally:
        h.close()
        front.close()
