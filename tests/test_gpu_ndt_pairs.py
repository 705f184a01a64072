"""Pairwise batch NDT on the GPU (locgpu_ndt_set_target_set*, locgpu_ndt_align_pairs, locgpu_ndt_fitness_pairs):
every scan of a batch against a voxel grid of its own. The reference for bits is the library's own ordinary path — an ordinary
context that holds ONE of the targets (locgpu_ndt_set_target, same options), locgpu_ndt_align_batch of the same batch, the scan's
row — and for poses the CPU oracle (locref.Ndt) per pair at the project's bar (1e-4 m / 1e-4 rad, equal iteration counts).

Set of the different-targets cases: [scan 0 … scan 4, a 20 000-point local map in scan 4's frame, five points in one voxel (one voxel
kept at min_pts_in_voxel = 3), four points in four voxels (no voxel kept: status 1, the init comes back)], voxel_size 2.0, NEARBY6.
At 2.0 the pairs (i, i−1) from the identity run 6, 6, 2, 6 and 13 iterations on the oracle (226 … 61 kept voxels); at 1.0 two of the
five stop after one iteration, which would test little."""
import numpy as np
import pytest

from conftest import pose_delta

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4
POSE_TOL_RAD = 1e-4
SIDS = (10, 11, 12, 13, 14, 15)
COUNTS = (4000, 3100, 2049, 1500, 900, 257)
TARGET_OF = (-1, 0, 1, 2, 5, 6)
FOUR = 7  # the four-point target
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
VOXEL = 2.0
MAX_ITERATION = 20  # the options' default: the oracle's cap
STATUS_ABORTED = 1  # det(H) == 0 (ndt_registration.cpp:435-436): the caller's pose stays


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_row(pose_a, st_a, pose_b, st_b, what):
    assert np.array_equal(_bits(pose_a), _bits(pose_b)), (what, pose_a, pose_b)
    for key in ("iterations", "converged", "status", "last_effective_num"):
        assert st_a[key] == st_b[key], (what, key, st_a, st_b)
    assert np.array_equal(_bits([st_a["last_dx_norm"]]), _bits([st_b["last_dx_norm"]])), (what, st_a, st_b)


def _same_fit(a, b, what):
    assert a["inliers"] == b["inliers"] and a["finite_points"] == b["finite_points"], (what, a, b)
    assert np.array_equal(_bits([a["score"]]), _bits([b["score"]])), (what, a, b)


def _yaw_pose(yaw, tx, ty):
    return np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2), tx, ty, 0.0])


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _sorted_dump(d):
    k, mu, info = d
    o = np.lexsort(k.T[::-1])
    return k[o], mu[o], info[o]


def _opts(api, **kw):
    kw.setdefault("voxel_size", VOXEL)
    kw.setdefault("nearby_type", 1)  # NEARBY6
    return api.ndt_opts(**kw)


@pytest.fixture(scope="module")
def set_ctx(api):
    api.lib()
    ctx = api.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def world(synth, locref):
    """Six consecutive scans of unequal counts in their sensor frames, a 20 000-point local map brought into scan 4's (perturbed) sensor
    frame so that the identity is a sensible start, five points in one voxel and four points in four voxels. The conditions the cases
    rely on are asserted from the oracle alone."""
    scans = [np.ascontiguousarray(synth.make_scan(s, subsample=n)[:, :3]) for s, n in zip(SIDS, COUNTS)]
    assert [len(s) for s in scans] == list(COUNTS)
    _, init4 = synth.make_pose(SIDS[4])
    m = synth.make_local_map(20000, SIDS[4], half=30.0)
    local = np.ascontiguousarray(((m[:, :3].astype(np.float64) - init4[4:]) @ _quat_R(init4[:4])).astype(np.float32))
    five = np.array([[5.0, 5.0, 1.0], [5.4, 5.1, 0.8], [4.7, 5.5, 1.2], [5.2, 4.6, 1.5], [4.9, 5.3, 0.5]], dtype=np.float32)
    four = np.array([[1.0, 1.0, 1.0], [3.0, 1.0, 1.0], [1.0, 3.0, 1.0], [1.0, 1.0, 3.0]], dtype=np.float32)
    targets = scans[:5] + [local, five, four]
    kept = []
    for t in targets:
        ndt = locref.Ndt(voxel_size=VOXEL)
        ndt.set_target(t)
        kept.append(ndt.num_voxels())
    assert all(k >= 50 for k in kept[:5]), kept
    assert kept[6] == 1 and kept[7] == 0, kept
    consecutive = {}
    for i in range(1, 6):
        ndt = locref.Ndt(voxel_size=VOXEL)
        ndt.set_target(scans[i - 1])
        r = ndt.align(scans[i], IDENTITY)
        assert r["status"] == 0 and 2 <= r["iters"] < MAX_ITERATION, (i, r["status"], r["iters"])
        consecutive[i] = r
    return dict(scans=scans, targets=targets, kept=kept, consecutive=consecutive)


def _per_pair(gpu_ctx, api, world, batch, inits, opts, target_of=TARGET_OF, rows=range(1, 6)):
    """Row i of locgpu_ndt_align_batch of the SAME six-scan batch on the ordinary context holding only target target_of[i]."""
    out = {}
    for i in rows:
        gpu_ctx.ndt_set_target(world["targets"][target_of[i]], opts)
        poses, stats = gpu_ctx.ndt_align_batch(batch, inits)
        out[i] = (poses[i].copy(), stats[i])
    return out


@pytest.fixture(scope="module")
def case3(gpu_ctx, set_ctx, api, locref, world):
    """Computed once: the pairs call with identity inits, the per-pair ordinary runs, the oracle per pair."""
    opts = _opts(api)
    set_ctx.ndt_set_target_set(world["targets"], opts)
    bs = set_ctx.batch(world["scans"])
    bo = gpu_ctx.batch(world["scans"])
    poses, stats = set_ctx.ndt_align_pairs(bs, TARGET_OF, None)
    inits = np.tile(IDENTITY, (6, 1))
    ordinary = _per_pair(gpu_ctx, api, world, bo, inits, opts)
    oracle = {}
    for i in range(1, 6):
        ndt = locref.Ndt(voxel_size=VOXEL)
        ndt.set_target(world["targets"][TARGET_OF[i]])
        oracle[i] = ndt.align(world["scans"][i], IDENTITY)
    yield dict(opts=opts, bs=bs, bo=bo, poses=poses, stats=stats, ordinary=ordinary, oracle=oracle, inits=inits)
    bs.close()
    bo.close()


# ------------------------------------------------------------------------------------------------ 1. set build against the single builds
def test_set_build_matches_single_builds(gpu_ctx, set_ctx, api, locref, world):
    opts = _opts(api)
    set_ctx.ndt_set_target_set(world["targets"], opts)
    info = set_ctx.ndt_set_info()
    assert info["n_targets"] == 8 and info["points"] == [len(t) for t in world["targets"]]
    assert info["voxels"] == world["kept"]
    assert set_ctx.ndt_target_info()["num_voxels"] == sum(world["kept"])
    first = [set_ctx.ndt_set_dump(j) for j in range(8)]
    for j, t in enumerate(world["targets"]):
        ks, mus, infos = first[j]
        assert np.array_equal(ks, _sorted_dump(first[j])[0]), j  # already in key order
        gpu_ctx.ndt_set_target(t, opts)
        kg, mug, ig = _sorted_dump(gpu_ctx.ndt_dump())
        assert len(ks) == gpu_ctx.ndt_target_info()["num_voxels"] == world["kept"][j]
        assert np.array_equal(ks, kg), j
        assert np.array_equal(_bits(mus), _bits(mug)) and np.array_equal(_bits(infos), _bits(ig)), j
        # ... and the oracle, the way test_ndt_voxel_table_matches_oracle compares: mu its bits, info through the same Jacobi on both sides
        ndt = locref.Ndt(voxel_size=VOXEL)
        ndt.set_target(t)
        ko, muo, io = _sorted_dump(ndt.dump())
        np.testing.assert_array_equal(ks, ko)
        np.testing.assert_array_equal(mus, muo)
        if len(ko):
            scale = np.abs(io).max(axis=(1, 2), keepdims=True)
            assert (np.abs(infos - io) / scale).max() < 1e-12, j
    # two ingests of the same set: the same dump bytes in the same order
    set_ctx.ndt_set_target_set(world["targets"], opts)
    for j in range(8):
        again = set_ctx.ndt_set_dump(j)
        for a, b in zip(first[j], again):
            assert a.tobytes() == b.tobytes(), j


# ------------------------------------------------------------------------------------------------ 2. same target in every slot
@pytest.mark.parametrize("nearby", [1, 0])
def test_same_target_in_every_slot(gpu_ctx, api, world, nearby):
    """The local map as targets 0…5, the scans dealt over them out of order: keys under target bits != 0 and collision walks among six
    copies of one grid, against the ordinary look-up in the one grid. NEARBY6 and CENTER."""
    local = world["targets"][5]
    opts = _opts(api, nearby_type=nearby)
    order = [3, 0, 5, 1, 4, 2]
    inits = np.tile(IDENTITY, (6, 1))
    inits[1, 4:] += [0.05, -0.05, 0.02]
    inits[2, 4:] -= [0.1, 0.0, 0.05]
    # every scan in scan 4's frame, so that each of them overlaps the map
    scans = [world["scans"][4][:n] for n in (900, 700, 513, 257, 64, 1)]
    c = api.Context(0)
    try:
        c.ndt_set_target_set([local] * 6, opts)
        gpu_ctx.ndt_set_target(local, opts)
        single = gpu_ctx.ndt_target_info()["num_voxels"]
        assert c.ndt_set_info()["voxels"] == [single] * 6
        bs, bo = c.batch(scans), gpu_ctx.batch(scans)
        ps, ss = c.ndt_align_pairs(bs, order, inits)
        po, so = gpu_ctx.ndt_align_batch(bo, inits)
        for i in range(6):
            _same_row(ps[i], ss[i], po[i], so[i], (nearby, i))
        assert ss[0]["iterations"] > 1 and ss[0]["last_effective_num"] > 100  # the comparison is of alignments that ran
        bs.close()
        bo.close()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 3. different targets
def test_different_targets(gpu_ctx, set_ctx, api, case3, world):
    poses, stats, oracle = case3["poses"], case3["stats"], case3["oracle"]
    for i in range(1, 6):
        po, so = case3["ordinary"][i]
        _same_row(poses[i], stats[i], po, so, i)
        ro = oracle[i]
        if ro["status"] == 0:
            assert stats[i]["status"] == 0, (i, stats[i])
        if ro["status"] == 0 and ro["iters"] < MAX_ITERATION:  # no bar for capped runs
            dt, dr = pose_delta(poses[i], ro["pose"])
            assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (i, dt, dr)
            assert stats[i]["iterations"] == ro["iters"], (i, stats[i], ro["iters"])
    # rows 1..3 are the consecutive pairs the fixture asserted: status 0, 2 <= iterations < 20
    for i in range(1, 4):
        assert oracle[i]["status"] == 0 and oracle[i]["iters"] == world["consecutive"][i]["iters"]
    # row 0 was given no target: its init pose, no iteration, the status that says so
    assert np.array_equal(_bits(poses[0]), _bits(IDENTITY))
    assert stats[0]["iterations"] == 0 and stats[0]["status"] == api.STATUS_NO_PAIR_TARGET == 5 and not stats[0]["converged"]
    assert all(stats[i]["status"] != api.STATUS_NO_PAIR_TARGET for i in range(1, 6))
    # a row against the four-point target, which keeps no voxel: det(H) == 0, status 1, the init comes back — as on the ordinary context
    inits = case3["inits"].copy()
    inits[0] = _yaw_pose(0.02, 0.1, -0.1)
    inits[5] = _yaw_pose(-0.03, 0.2, 0.1)
    target_of = (FOUR, -1, -1, -1, -1, FOUR)
    p4, s4 = set_ctx.ndt_align_pairs(case3["bs"], target_of, inits)
    want = _per_pair(gpu_ctx, api, world, case3["bo"], inits, case3["opts"], target_of=target_of, rows=(0, 5))
    for i in (0, 5):
        _same_row(p4[i], s4[i], want[i][0], want[i][1], ("four", i))
        assert s4[i]["status"] == STATUS_ABORTED and np.array_equal(_bits(p4[i]), _bits(inits[i])), (i, s4[i])
    assert all(s4[i]["status"] == api.STATUS_NO_PAIR_TARGET for i in range(1, 5))


# ------------------------------------------------------------------------------------------------ 4. the pts branches
def test_points_per_thread_branch(gpu_ctx, api, synth, world):
    """32 scans of 16 384 points: 64 blocks x 32 scans = 2048 block rows, the smallest shape that takes pts = 2 — where a wrong pts
    rule or partial layout of the pairs launcher shows."""
    n, cnt = 32, 16384
    local = world["targets"][5]
    opts = _opts(api)
    base = np.ascontiguousarray(synth.make_scan(SIDS[4])[:, :3])
    assert len(base) >= cnt
    rng = np.random.default_rng(7)
    scans = [np.ascontiguousarray(base[np.sort(rng.choice(len(base), cnt, replace=False))]) for _ in range(n)]
    inits = np.tile(IDENTITY, (n, 1))
    inits[:, 4:] += rng.uniform(-0.1, 0.1, (n, 3))
    c = api.Context(0)
    try:
        c.ndt_set_target_set([local] * n, opts)
        gpu_ctx.ndt_set_target(local, opts)
        bs, bo = c.batch(scans), gpu_ctx.batch(scans)
        ps, ss = c.ndt_align_pairs(bs, list(range(n))[::-1], inits)
        po, so = gpu_ctx.ndt_align_batch(bo, inits)
        for i in range(n):
            _same_row(ps[i], ss[i], po[i], so[i], i)
        assert all(s["iterations"] >= 1 and s["last_effective_num"] == cnt for s in ss)
        assert any(s["iterations"] > 1 for s in ss)
        bs.close()
        bo.close()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 5. open-scan compaction
OPEN_INITS = np.stack([IDENTITY, _yaw_pose(0.03, 0.3, 0.2), _yaw_pose(-0.02, -0.3, 0.25), IDENTITY, _yaw_pose(0.02, 0.25, -0.2), IDENTITY])


def test_open_scan_compaction(gpu_ctx, set_ctx, api, locref, case3, world):
    """Inits under which, by the oracle's own iteration counts, some pairs end within the first chunk of 8 iterations and others
    need more: the later chunks of the pairs call against those of the ordinary runs."""
    inits = OPEN_INITS
    iters = {}
    for i in range(1, 6):
        ndt = locref.Ndt(voxel_size=VOXEL)
        ndt.set_target(world["targets"][TARGET_OF[i]])
        iters[i] = ndt.align(world["scans"][i], inits[i])["iters"]
    assert any(n <= 8 for n in iters.values()) and any(n > 8 for n in iters.values()), iters
    assert any(8 < n < MAX_ITERATION for n in iters.values()), iters  # one that needs a later chunk and leaves before the cap
    poses, stats = set_ctx.ndt_align_pairs(case3["bs"], TARGET_OF, inits)
    ordinary = _per_pair(gpu_ctx, api, world, case3["bo"], inits, case3["opts"])
    for i in range(1, 6):
        _same_row(poses[i], stats[i], ordinary[i][0], ordinary[i][1], i)
        if iters[i] < MAX_ITERATION:
            assert stats[i]["iterations"] == iters[i], (i, stats[i], iters)
    assert np.array_equal(_bits(poses[0]), _bits(inits[0])) and stats[0]["iterations"] == 0


# ------------------------------------------------------------------------------------------------ 6. set from a batch
def test_set_from_a_batch(api, world):
    order = [-1, 0, 1, 2, 3, 4]
    opts = _opts(api)
    a, b = api.Context(0), api.Context(0)
    try:
        ba = a.batch(world["scans"])
        counts, status = ba.preprocess(0.5)
        assert (status == 0).all() and (counts > 0).all() and (counts < np.array(COUNTS)).any()
        a.ndt_set_target_set_batch(ba, opts)
        down = [np.ascontiguousarray(np.asarray(ba.download_scan(s))[:, :3]) for s in range(6)]
        assert [len(d) for d in down] == list(counts)
        b.ndt_set_target_set(down, opts)
        ia, ib = a.ndt_set_info(), b.ndt_set_info()
        assert ia == ib and ia["n_targets"] == 6 and ia["points"] == list(counts)
        for j in range(6):
            for x, y in zip(a.ndt_set_dump(j), b.ndt_set_dump(j)):
                assert x.tobytes() == y.tobytes(), j
        # the batch the set was built from is the source of the pairs call; a fresh batch of the same scans gives the same poses
        pa, sa = a.ndt_align_pairs(ba, order, None)
        bb = b.batch(down)
        pb, sb = b.ndt_align_pairs(bb, order, None)
        for i in range(6):
            _same_row(pa[i], sa[i], pb[i], sb[i], i)
        assert sa[1]["iterations"] > 0 and sa[0]["status"] == api.STATUS_NO_PAIR_TARGET
        ba.close()
        bb.close()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 7. the range boundary
def test_range_boundary(gpu_ctx, api, world):
    """A query in voxel x = 32768, just outside the set's ±2^15 range, whose face neighbour x = 32767 is inside and holds the target:
    the ordinary path (range ±2^20) probes it, and so must the pairs kernels."""
    opts = _opts(api, voxel_size=1.0, res_outlier_th=1e6)
    rng = np.random.default_rng(5)
    edge = np.empty((8, 3), dtype=np.float32)
    edge[:, 0] = 32767.0 + rng.uniform(0.1, 0.9, 8)
    edge[:, 1:] = rng.uniform(0.1, 0.9, (8, 2))
    assert np.linalg.matrix_rank((edge - edge.mean(0)).astype(np.float64)) == 3  # non-coplanar
    src = np.empty((20, 3), dtype=np.float32)
    src[:, 0] = 32768.0 + rng.uniform(0.1, 0.9, 20)
    src[:, 1:] = rng.uniform(0.1, 0.9, (20, 2))
    assert (np.floor(edge[:, 0].astype(np.float64)) == 32767).all() and (np.floor(src[:, 0].astype(np.float64)) == 32768).all()
    near = np.ascontiguousarray(world["scans"][0][np.abs(world["scans"][0]).max(axis=1) < 30.0])  # voxel 1.0: well inside the range
    scans = [src, world["scans"][1]]
    inits = np.tile(IDENTITY, (2, 1))
    c = api.Context(0)
    try:
        c.ndt_set_target_set([edge, near], opts)
        bs, bo = c.batch(scans), gpu_ctx.batch(scans)
        ps, ss = c.ndt_align_pairs(bs, [0, 1], inits)
        fs = c.ndt_fitness_pairs(bs, [0, 1], inits)
        for i, t in enumerate((edge, near)):
            gpu_ctx.ndt_set_target(t, opts)
            po, so = gpu_ctx.ndt_align_batch(bo, inits)
            fo = gpu_ctx.ndt_fitness_batch(bo, inits)
            _same_row(ps[i], ss[i], po[i], so[i], i)
            _same_fit(fs[i], fo[i], i)
            if i == 0:
                assert fo[0]["inliers"] >= 1 and fo[0]["finite_points"] == 20, fo[0]  # the probe across the boundary was really taken
        # a target with a point beyond the range is refused by index, and the previous set still answers
        beyond = np.vstack([edge, np.array([[32768.5, 0.5, 0.5]], dtype=np.float32)])
        with pytest.raises(api.LocGpuError) as e:
            c.ndt_set_target_set([near, beyond], opts)
        assert e.value.code == -1 and "target 1" in str(e.value), str(e.value)
        assert c.ndt_set_info()["points"] == [8, len(near)]
        ps2, ss2 = c.ndt_align_pairs(bs, [0, 1], inits)
        for i in range(2):
            _same_row(ps2[i], ss2[i], ps[i], ss[i], i)
        bs.close()
        bo.close()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 8. fitness per pair
def test_fitness_pairs(gpu_ctx, set_ctx, api, case3, world):
    poses = case3["poses"]
    fit = set_ctx.ndt_fitness_pairs(case3["bs"], TARGET_OF, poses)
    for i in range(1, 6):
        gpu_ctx.ndt_set_target(world["targets"][TARGET_OF[i]], case3["opts"])
        want = gpu_ctx.ndt_fitness_batch(case3["bo"], poses)[i]
        _same_fit(fit[i], want, i)
    assert any(fit[i]["inliers"] > 100 for i in range(1, 6))
    assert fit[0]["score"] == np.inf and fit[0]["inliers"] == 0 and fit[0]["finite_points"] == 0


# ------------------------------------------------------------------------------------------------ 9. refusals, return to ordinary
def test_refusals_and_return_to_ordinary(gpu_ctx, api, world):
    opts = _opts(api)
    icp = api.icp_opts(method=api.P2PLANE)
    inits = np.tile(IDENTITY, (6, 1))
    c = api.Context(0)
    try:
        c.icp_set_target(world["targets"][5])
        c.ndt_set_target(world["targets"][5], opts)
        pool = api.Pool(c, 4, 4096, ndt=True)  # made against an ordinary target: its re-check at submit meets the set
        c.ndt_set_target_set(world["targets"], opts)
        b = c.batch(world["scans"])
        before = [np.asarray(b.download_scan(s)).copy() for s in range(6)]
        info = c.ndt_set_info()
        for bad in ([-1, 0, 1, 2, 5, 8], [-2, 0, 1, 2, 5, 6]):
            with pytest.raises(api.LocGpuError) as e:
                c.ndt_align_pairs(b, bad, None)
            assert e.value.code == -1 and "target_of" in str(e.value)
            with pytest.raises(api.LocGpuError) as e:
                c.ndt_fitness_pairs(b, bad, inits)
            assert e.value.code == -1 and "target_of" in str(e.value)
        # a set context answers only the pairs calls
        scan = world["scans"][1]
        calls = dict(
            ndt_align_batch=lambda: c.ndt_align_batch(b, inits), ndt_align_batch_begin=lambda: c.ndt_align_batch_begin(b, inits),
            ndt_align=lambda: c.ndt_align(scan, IDENTITY), ndt_hb=lambda: c.ndt_hb(scan, IDENTITY), ndt_hb_batch=lambda: c.ndt_hb_batch(b, inits),
            ndt_scan_match=lambda: c.ndt_scan_match(scan, IDENTITY), ndt_fitness=lambda: c.ndt_fitness(scan, IDENTITY),
            ndt_fitness_batch=lambda: c.ndt_fitness_batch(b, inits), ndt_fitness_resident=lambda: c.ndt_fitness_resident(IDENTITY),
            ndt_init_search=lambda: c.ndt_init_search(scan, inits), ndt_dump=lambda: c.ndt_dump(),
            pool=lambda: api.Pool(c, 4, 4096, ndt=True))
        for name, call in calls.items():
            with pytest.raises(api.LocGpuError) as e:
                call()
            assert e.value.code == -1 and "voxel-set" in str(e.value), (name, str(e.value))
        with pytest.raises(api.LocGpuError) as e:
            pool.submit([world["scans"][1]], [IDENTITY])
        assert e.value.code == -1 and "voxel-set" in str(e.value), str(e.value)
        pool.close()
        # refusals of the ingest: the incremental method, an empty target (by index), too many or no targets — the set stays
        with pytest.raises(api.LocGpuError) as e:
            c.ndt_set_target_set(world["targets"], _opts(api, method=2))
        assert e.value.code == -1 and "incremental" in str(e.value)
        with pytest.raises(api.LocGpuError) as e:
            c.ndt_set_target_set([world["targets"][0], np.zeros((0, 3), np.float32), world["targets"][1]], opts)
        assert e.value.code == -1 and "target 1" in str(e.value)
        with pytest.raises(api.LocGpuError) as e:
            c.ndt_set_target_set([], opts)
        assert e.value.code == -1
        # batches the pairs calls and the batch ingest do not take: another context's, sharded, shared-source, one with an alignment in flight
        gpu_ctx.ndt_set_target(world["targets"][5], opts)
        bo = gpu_ctx.batch(world["scans"])
        shared = c.batch_shared(world["scans"][0], 6)
        sharded = c.batch(world["scans"], first=0, n_total=6)  # one rank holding every scan: sharded all the same
        for other in (bo, shared, sharded):
            with pytest.raises(api.LocGpuError) as e:
                c.ndt_align_pairs(other, TARGET_OF, None)
            assert e.value.code == -1
            with pytest.raises(api.LocGpuError) as e:
                c.ndt_fitness_pairs(other, TARGET_OF, inits)
            assert e.value.code == -1
            with pytest.raises(api.LocGpuError) as e:
                c.ndt_set_target_set_batch(other, opts)
            assert e.value.code == -1
        c.icp_align_batch_begin(b, inits, icp)  # the ICP target is untouched: an ICP alignment in flight on the batch
        for call in (lambda: c.ndt_align_pairs(b, TARGET_OF, None), lambda: c.ndt_fitness_pairs(b, TARGET_OF, inits), lambda: c.ndt_set_target_set_batch(b, opts)):
            with pytest.raises(api.LocGpuError) as e:
                call()
            assert e.value.code == -1 and "begun" in str(e.value)
        c.align_batch_end(b)
        assert c.ndt_set_info() == info
        for s in range(6):
            assert np.array_equal(np.asarray(b.download_scan(s)), before[s])
        # an ordinary context refuses the pairs calls
        with pytest.raises(api.LocGpuError) as e:
            gpu_ctx.ndt_align_pairs(bo, [0] * 6, None)
        assert e.value.code == -1 and "ordinary" in str(e.value)
        with pytest.raises(api.LocGpuError) as e:
            gpu_ctx.ndt_fitness_pairs(bo, [0] * 6, inits)
        assert e.value.code == -1 and "ordinary" in str(e.value)
        with pytest.raises(api.LocGpuError):
            gpu_ctx.ndt_set_info()
        with pytest.raises(api.LocGpuError):
            gpu_ctx.ndt_set_dump(0)
        # the set context still aligns in pairs after all of this
        ps, ss = c.ndt_align_pairs(b, TARGET_OF, None)
        assert ss[1]["iterations"] > 0 and ss[0]["status"] == api.STATUS_NO_PAIR_TARGET
        # back to ordinary: the bits an untouched context returns
        want_p, want_s = gpu_ctx.ndt_align_batch(bo, inits)
        c.ndt_set_target(world["targets"][5], opts)
        got_p, got_s = c.ndt_align_batch(b, inits)
        for i in range(6):
            _same_row(got_p[i], got_s[i], want_p[i], want_s[i], i)
        assert c.ndt_target_info() == gpu_ctx.ndt_target_info()
        with pytest.raises(api.LocGpuError):
            c.ndt_align_pairs(b, TARGET_OF, None)
        # the ICP target the context held throughout still answers
        gpu_ctx.icp_set_target(world["targets"][5])
        wi_p, wi_s = gpu_ctx.icp_align_batch(bo, inits, icp)
        gi_p, gi_s = c.icp_align_batch(b, inits, icp)
        for i in range(6):
            _same_row(gi_p[i], gi_s[i], wi_p[i], wi_s[i], ("icp", i))
        for x in (b, bo, shared, sharded):
            x.close()
    finally:
        c.close()
