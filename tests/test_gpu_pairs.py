"""Pairwise batch ICP on the GPU (locgpu_icp_set_target_forest*, locgpu_icp_align_pairs, locgpu_icp_fitness_pairs):
every scan of a batch against a target of its own. The reference for bits is the library's own ordinary path — an ordinary context
that holds ONE of the targets, locgpu_icp_align_batch of the same batch, the scan's row — and for poses the CPU oracle per pair at
the project's bar (1e-4 m / 1e-4 rad, equal iteration counts where the oracle left before its cap).

Forest of the different-targets cases: [scan 0 … scan 4, a 20 000-point local map, a target of exactly 5 points], seven trees, so that
target_of = [-1, 0, 1, 2, 5, 6] reads the first and the last segment, trees of depth 4 … 19 and the k = 5 boundary (5 leaves)."""
import numpy as np
import pytest

from conftest import pose_delta

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4
POSE_TOL_RAD = 1e-4
SIDS = (10, 11, 12, 13, 14, 15)
COUNTS = (4000, 3100, 2049, 1500, 900, 257)
TARGET_OF = (-1, 0, 1, 2, 5, 6)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
MAX_ITERATION = 20  # the options' default: the oracle's cap


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_row(pose_a, st_a, pose_b, st_b, what):
    assert np.array_equal(_bits(pose_a), _bits(pose_b)), (what, pose_a, pose_b)
    for key in ("iterations", "converged", "status", "last_effective_num"):
        assert st_a[key] == st_b[key], (what, key, st_a, st_b)
    assert np.array_equal(_bits([st_a["last_dx_norm"]]), _bits([st_b["last_dx_norm"]])), (what, st_a, st_b)


def _yaw_pose(yaw, tx, ty):
    return np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2), tx, ty, 0.0])


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.fixture(scope="module")
def forest_ctx(api):
    api.lib()
    ctx = api.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def world(synth):
    """Six consecutive scans of unequal counts in their sensor frames, a 20 000-point local map brought into scan 4's (perturbed) sensor
    frame so that the identity is a sensible start, and a target of the first five points of scan 5."""
    scans = [np.ascontiguousarray(synth.make_scan(s, subsample=n)[:, :3]) for s, n in zip(SIDS, COUNTS)]
    assert [len(s) for s in scans] == list(COUNTS)
    _, init4 = synth.make_pose(SIDS[4])
    m = synth.make_local_map(20000, SIDS[4], half=30.0)
    local = np.ascontiguousarray(((m[:, :3].astype(np.float64) - init4[4:]) @ _quat_R(init4[:4])).astype(np.float32))
    five = np.ascontiguousarray(scans[5][:5])
    assert len(np.unique(five, axis=0)) == 5
    targets = scans[:5] + [local, five]
    return dict(scans=scans, targets=targets)


def _per_pair(gpu_ctx, api, world, batch, inits, opts, rows=range(1, 6)):
    """Row i of locgpu_icp_align_batch of the SAME six-scan batch on the ordinary context holding only target TARGET_OF[i]."""
    out = {}
    for i in rows:
        gpu_ctx.icp_set_target(world["targets"][TARGET_OF[i]])
        poses, stats = gpu_ctx.icp_align_batch(batch, inits, opts)
        out[i] = (poses[i].copy(), stats[i])
    return out


@pytest.fixture(scope="module")
def case2(gpu_ctx, forest_ctx, api, locref, world):
    """Computed once: the pairs call with identity inits, the per-pair ordinary runs, the oracle per pair."""
    opts = api.icp_opts(method=api.P2PLANE)
    forest_ctx.icp_set_target_forest(world["targets"])
    bf = forest_ctx.batch(world["scans"])
    bo = gpu_ctx.batch(world["scans"])
    poses, stats = forest_ctx.icp_align_pairs(bf, TARGET_OF, None, opts)
    inits = np.tile(IDENTITY, (6, 1))
    ordinary = _per_pair(gpu_ctx, api, world, bo, inits, opts)
    oracle = {}
    for i in range(1, 6):
        icp = locref.Icp(method=locref.P2PLANE)
        icp.set_target(world["targets"][TARGET_OF[i]])
        oracle[i] = icp.align(world["scans"][i], IDENTITY)
    yield dict(opts=opts, bf=bf, bo=bo, poses=poses, stats=stats, ordinary=ordinary, oracle=oracle)
    bf.close()
    bo.close()


# ------------------------------------------------------------------------------------------------ 1. same target in every slot
@pytest.mark.parametrize("method", [2, 1, 0])
def test_same_target_in_every_slot(gpu_ctx, api, synth, method):
    """Four copies of one 20 000-point map as the forest, scans of 4113, 257, 64 and 1 points: the one-thread-per-query route over
    segments at base != 0 against the ordinary search route on the one map — neighbour lists index for index after the first
    iteration, poses and every stats field bit for bit."""
    sid = 5
    m = synth.make_local_map(20000, sid, half=25.0)
    scans = [synth.make_scan(sid, subsample=n, crop_half=22.0) for n in (4113, 257, 64, 1)]
    assert [len(s) for s in scans] == [4113, 257, 64, 1]
    _, init = synth.make_pose(sid)
    inits = np.tile(init, (4, 1))
    inits[1, 4:] += [0.05, -0.05, 0.02]
    inits[2, 4:] -= [0.1, 0.0, 0.05]
    k = 1 if method == 0 else 5
    fctx = api.Context(0)
    try:
        fctx.icp_set_target_forest([m, m, m, m])
        info = fctx.icp_forest_info()
        gpu_ctx.icp_set_target(m)
        single = gpu_ctx.icp_target_info()
        assert info["n_targets"] == 4 and info["leaves"] == [single["num_leaves"]] * 4 and info["depth"] == [single["depth"]] * 4
        bf, bo = fctx.batch(scans), gpu_ctx.batch(scans)
        one = api.icp_opts(method=method, max_iteration=1)
        fctx.icp_align_pairs(bf, [0, 1, 2, 3], inits, one)
        gpu_ctx.icp_align_batch(bo, inits, one)
        nn_f, nn_o = fctx.debug_batch_nn(bf, k), gpu_ctx.debug_batch_nn(bo, k)
        for i, s in enumerate(scans):
            assert np.array_equal(nn_f[i, :len(s)], nn_o[i, :len(s)]), (method, i)
            assert (nn_f[i, :len(s)] >= 0).all() and (nn_f[i, :len(s)] < len(m)).all()
        opts = api.icp_opts(method=method)
        pf, sf = fctx.icp_align_pairs(bf, [0, 1, 2, 3], inits, opts)
        po, so = gpu_ctx.icp_align_batch(bo, inits, opts)
        for i in range(4):
            _same_row(pf[i], sf[i], po[i], so[i], (method, i))
        assert sf[0]["iterations"] > 1 and sf[0]["last_effective_num"] > 100  # the comparison is of alignments that ran
        bf.close()
        bo.close()
    finally:
        fctx.close()


def test_same_target_against_the_walk_deep_and_redo_route(gpu_ctx, api, synth):
    """The four-scan batches above are small enough for the ordinary context's one-launch 16-lane search. 32 scans of 4113 points are
    2080 waves, past the 2048 below which that shortcut is taken: the ordinary side now runs the 64-lane walk kernel with its deep
    and redo passes (it reports run flags, which only that route writes) — and the pairs route must still give its bits, from 32
    segments."""
    sid, n = 5, 32
    m = synth.make_local_map(20000, sid, half=25.0)
    scan = synth.make_scan(sid, subsample=4113, crop_half=22.0)
    _, init = synth.make_pose(sid)
    inits = np.tile(init, (n, 1))
    rng = np.random.default_rng(3)
    inits[:, 4:] += rng.uniform(-0.15, 0.15, (n, 3))
    # six iterations: all inside the first chunk, which launches every scan of the batch (a later chunk over a few open scans would
    # fall below the 2048 waves again)
    opts = api.icp_opts(method=api.P2PLANE, max_iteration=6)
    fctx = api.Context(0)
    try:
        fctx.icp_set_target_forest([m] * n)
        gpu_ctx.icp_set_target(m)
        bf, bo = fctx.batch([scan] * n), gpu_ctx.batch([scan] * n)
        pf, sf = fctx.icp_align_pairs(bf, list(range(n)), inits, opts)
        po, so = gpu_ctx.icp_align_batch(bo, inits, opts)
        assert gpu_ctx.debug_batch_run_flags(bo)[1] and not fctx.debug_batch_run_flags(bf)[1]
        for i in range(n):
            _same_row(pf[i], sf[i], po[i], so[i], i)
        assert all(1 < s["iterations"] <= 6 and s["last_effective_num"] > 100 for s in sf)
        bf.close()
        bo.close()
    finally:
        fctx.close()


# ------------------------------------------------------------------------------------------------ 2. different targets
def test_different_targets(api, case2, world):
    poses, stats, oracle = case2["poses"], case2["stats"], case2["oracle"]
    for i in range(1, 6):
        po, so = case2["ordinary"][i]
        _same_row(poses[i], stats[i], po, so, i)
        ro = oracle[i]
        if ro["iters"] < MAX_ITERATION:  # no bar for capped runs
            dt, dr = pose_delta(poses[i], ro["pose"])
            assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (i, dt, dr)
            assert stats[i]["iterations"] == ro["iters"], (i, stats[i], ro["iters"])
    assert any(oracle[i]["iters"] < MAX_ITERATION for i in range(1, 6))
    # row 0 was given no target: its init pose, no iteration, the status that says so
    assert np.array_equal(_bits(poses[0]), _bits(IDENTITY))
    assert stats[0]["iterations"] == 0 and stats[0]["status"] == api.STATUS_NO_PAIR_TARGET and not stats[0]["converged"]
    assert all(stats[i]["status"] != api.STATUS_NO_PAIR_TARGET for i in range(1, 6))


def test_pairs_neighbours_are_each_targets_own_points(forest_ctx, api, case2, world, locref):
    """locgpu_debug_batch_nn after a pairs call: per-target point indices — the oracle tree's exact 5-NN of each pair at the identity."""
    one = api.icp_opts(method=api.P2PLANE, max_iteration=1, approximate=0)
    forest_ctx.icp_align_pairs(case2["bf"], TARGET_OF, None, one)
    nn = forest_ctx.debug_batch_nn(case2["bf"], 5)
    for i in range(1, 6):
        target, scan = world["targets"][TARGET_OF[i]], world["scans"][i]
        tree = locref.KdTree(target)
        want = tree.knn(scan, 5, approximate=False)
        assert np.array_equal(nn[i, :len(scan)], np.asarray(want).reshape(len(scan), 5)), i


# ------------------------------------------------------------------------------------------------ 3. open-scan compaction
def test_open_scan_compaction(gpu_ctx, forest_ctx, api, locref, case2, world):
    """Inits under which, by the oracle's own iteration counts, some pairs end within the first chunk of 8 iterations and others
    need more: later chunks run over the open scans only (the active / n_active route of the pairs kernel)."""
    inits = np.stack([IDENTITY, _yaw_pose(0.1, 1.0, 0.5), _yaw_pose(-0.08, -1.2, 0.8), IDENTITY, _yaw_pose(0.05, 0.8, -0.6), IDENTITY])
    iters = {}
    for i in range(1, 6):
        icp = locref.Icp(method=locref.P2PLANE)
        icp.set_target(world["targets"][TARGET_OF[i]])
        iters[i] = icp.align(world["scans"][i], inits[i])["iters"]
    assert any(n <= 8 for n in iters.values()) and any(n > 8 for n in iters.values()), iters
    assert any(8 < n < MAX_ITERATION for n in iters.values()), iters  # one that needs a later chunk and leaves before the cap
    poses, stats = forest_ctx.icp_align_pairs(case2["bf"], TARGET_OF, inits, case2["opts"])
    ordinary = _per_pair(gpu_ctx, api, world, case2["bo"], inits, case2["opts"])
    for i in range(1, 6):
        _same_row(poses[i], stats[i], ordinary[i][0], ordinary[i][1], i)
        if iters[i] < MAX_ITERATION:
            assert stats[i]["iterations"] == iters[i], (i, stats[i], iters)
    assert np.array_equal(_bits(poses[0]), _bits(inits[0])) and stats[0]["iterations"] == 0


# ------------------------------------------------------------------------------------------------ 4. forest from a batch
def test_forest_from_a_batch(api, world, locref):
    order = [-1, 0, 1, 2, 3, 4]
    opts = api.icp_opts(method=api.P2PLANE)
    a, b = api.Context(0), api.Context(0)
    try:
        ba = a.batch(world["scans"])
        a.icp_set_target_forest_batch(ba)
        pa, sa = a.icp_align_pairs(ba, order, None, opts)
        down = [ba.download_scan(s) for s in range(6)]
        for s in range(6):
            assert np.array_equal(np.asarray(down[s])[:, :3], world["scans"][s])
        b.icp_set_target_forest([np.ascontiguousarray(np.asarray(d)[:, :3]) for d in down])
        bb = b.batch(world["scans"])
        pb, sb = b.icp_align_pairs(bb, order, None, opts)
        for i in range(6):
            _same_row(pa[i], sa[i], pb[i], sb[i], i)
        ia, ib = a.icp_forest_info(), b.icp_forest_info()
        assert ia == ib and ia["n_targets"] == 6
        for s in range(6):
            icp = locref.Icp(method=locref.P2PLANE)
            icp.set_target(world["scans"][s])
            t = icp.tree_info()
            assert ia["leaves"][s] == t["num_leaves"] and ia["depth"][s] == t["depth"], s
        assert sa[1]["iterations"] > 0 and sa[0]["status"] == api.STATUS_NO_PAIR_TARGET
        ba.close()
        bb.close()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 5. score
def test_fitness_pairs(gpu_ctx, forest_ctx, api, case2, world):
    poses = case2["poses"]
    fit = forest_ctx.icp_fitness_pairs(case2["bf"], TARGET_OF, poses, 1.0)
    for i in range(1, 6):
        gpu_ctx.icp_set_target(world["targets"][TARGET_OF[i]])
        want = gpu_ctx.icp_fitness_batch(case2["bo"], poses, 1.0)[i]
        assert fit[i]["inliers"] == want["inliers"] and fit[i]["finite_points"] == want["finite_points"], (i, fit[i], want)
        assert np.array_equal(_bits([fit[i]["score"]]), _bits([want["score"]])), (i, fit[i], want)
    assert any(fit[i]["inliers"] > 100 for i in range(1, 6))
    assert fit[0]["score"] == np.inf and fit[0]["inliers"] == 0


# ------------------------------------------------------------------------------------------------ 6. refusals, return to ordinary
def test_refusals_and_return_to_ordinary(gpu_ctx, api, world):
    opts = api.icp_opts(method=api.P2PLANE)
    inits = np.tile(IDENTITY, (6, 1))
    c = api.Context(0)
    try:
        c.icp_set_target_forest(world["targets"])
        b = c.batch(world["scans"])
        before = [np.asarray(b.download_scan(s)).copy() for s in range(6)]
        for bad in ([-1, 0, 1, 2, 5, 7], [-2, 0, 1, 2, 5, 6]):
            with pytest.raises(api.LocGpuError) as e:
                c.icp_align_pairs(b, bad, None, opts)
            assert e.value.code == -1 and "target_of" in str(e.value)
            with pytest.raises(api.LocGpuError) as e:
                c.icp_fitness_pairs(b, bad, inits, 1.0)
            assert e.value.code == -1 and "target_of" in str(e.value)
        for s in range(6):
            assert np.array_equal(np.asarray(b.download_scan(s)), before[s])
        # a forest context answers only the pairs calls
        with pytest.raises(api.LocGpuError) as e:
            c.icp_align_batch(b, inits, opts)
        assert e.value.code == -1 and "forest" in str(e.value)
        with pytest.raises(api.LocGpuError) as e:
            c.knn(world["scans"][0][:10], k=1)
        assert e.value.code == -1 and "forest" in str(e.value)
        with pytest.raises(api.LocGpuError) as e:
            c.icp_fitness_batch(b, inits, 1.0)
        assert e.value.code == -1 and "forest" in str(e.value)
        for o in (api.icp_opts(method=api.P2PLANE_MAP), api.icp_opts(method=api.P2PLANE, search_mode=api.SEARCH_GRID_EXACT)):
            with pytest.raises(api.LocGpuError) as e:
                c.icp_align_pairs(b, TARGET_OF, None, o)
            assert e.value.code == -1
        # an ordinary context refuses the pairs calls
        gpu_ctx.icp_set_target(world["targets"][5])
        bo = gpu_ctx.batch(world["scans"])
        with pytest.raises(api.LocGpuError) as e:
            gpu_ctx.icp_align_pairs(bo, [0] * 6, None, opts)
        assert e.value.code == -1 and "ordinary" in str(e.value)
        with pytest.raises(api.LocGpuError) as e:
            gpu_ctx.icp_fitness_pairs(bo, [0] * 6, inits, 1.0)
        assert e.value.code == -1 and "ordinary" in str(e.value)
        with pytest.raises(api.LocGpuError):
            gpu_ctx.icp_forest_info()
        # a batch of another context
        with pytest.raises(api.LocGpuError) as e:
            c.icp_align_pairs(bo, TARGET_OF, None, opts)
        assert e.value.code == -1
        # back to ordinary: the bits an untouched context returns
        want_p, want_s = gpu_ctx.icp_align_batch(bo, inits, opts)
        c.icp_set_target(world["targets"][5])
        got_p, got_s = c.icp_align_batch(b, inits, opts)
        for i in range(6):
            _same_row(got_p[i], got_s[i], want_p[i], want_s[i], i)
        assert c.icp_target_info() == gpu_ctx.icp_target_info()
        with pytest.raises(api.LocGpuError):
            c.icp_align_pairs(b, TARGET_OF, None, opts)
        b.close()
        bo.close()
    finally:
        c.close()
