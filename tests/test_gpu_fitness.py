"""The fitness score (include/locgpu.h: locgpu_icp_fitness, locgpu_icp_fitness_batch) against its definition restated with the
oracle's transform, the oracle's EXACT k = 1 tree search and numpy: counts equal, the FP64 sum within 1e-9 relative (the bar
test_icp_hb_matches_oracle sets for FP64 sums whose order differs)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-9


def _d2(q, nb):
    d = q - nb
    return d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])  # float32, the search's grouping, no contraction


def _queries(locref, scan, pose):
    p = np.ascontiguousarray(scan[:, :3], dtype=np.float32)
    fin = np.isfinite(p).all(axis=1)
    return locref.transform_points(pose, p[fin].astype(np.float64)).astype(np.float32)


def _expected(locref, tree, map_xyz, scan, pose, max_range, clear_of_gate=True):
    q = _queries(locref, scan, pose)
    idx = tree.knn(q, k=1, approximate=False)[:, 0]
    d2 = _d2(q, map_xyz[idx])
    assert d2.dtype == np.float32
    gate = np.float32(max_range * max_range)
    if clear_of_gate and np.isfinite(gate):
        assert np.abs(d2.astype(np.float64) - float(gate)).min() > 1e-5  # no point sits on the gate: the counts are unambiguous
    inl = d2 <= gate
    n_inl = int(inl.sum())
    score = float(d2[inl].astype(np.float64).sum() / n_inl) if n_inl else float("inf")
    return dict(score=score, inliers=n_inl, finite_points=len(q)), d2


def _brute_d2(q, map_xyz):
    out = np.empty(len(q), np.float32)
    mx, my, mz = (np.ascontiguousarray(map_xyz[:, a]) for a in range(3))
    for lo in range(0, len(q), 64):
        c = q[lo:lo + 64]
        dx, dy, dz = c[:, None, 0] - mx[None, :], c[:, None, 1] - my[None, :], c[:, None, 2] - mz[None, :]
        out[lo:lo + 64] = (dx * dx + (dy * dy + dz * dz)).min(axis=1)
    return out


def _check(got, want):
    print("fitness: got %r want %r rel %.3e" % (got, want, abs(got["score"] - want["score"]) / want["score"] if np.isfinite(want["score"]) else 0.0))
    assert got["inliers"] == want["inliers"] and got["finite_points"] == want["finite_points"], (got, want)
    if np.isfinite(want["score"]):
        assert abs(got["score"] - want["score"]) <= SUM_RTOL * want["score"], (got, want)
    else:
        assert got["score"] == float("inf")


@pytest.fixture(scope="module")
def world(synth, locref, gpu_ctx):
    m = synth.make_local_map(200_000, 7, half=40)
    s = synth.make_scan(7, crop_half=30, subsample=4000)
    true_pose, init_pose = synth.make_pose(7)
    tree = locref.KdTree(m)
    gpu_ctx.icp_set_target(m)
    return dict(map=np.ascontiguousarray(m[:, :3]), scan=s, true=true_pose, init=init_pose, tree=tree)


def _more_poses(synth, true_pose):
    a = true_pose.copy(); a[4:] += [0.7, -0.4, 0.05]
    _, b = synth.make_pose(7, trans_amp=1.0, rot_amp_deg=5.0)
    return [a, b]


def test_fitness_matches_definition(api, gpu_ctx, locref, synth, world):
    assert len(world["scan"]) == 4000
    for name, pose in [("true", world["true"]), ("perturbed", world["init"])] + [("more", p) for p in _more_poses(synth, world["true"])]:
        want, d2 = _expected(locref, world["tree"], world["map"], world["scan"], pose, 1.0)
        if name in ("true", "perturbed"):
            # the expectation itself: the exact tree's distances are the brute-force minima over all 200 000 map points
            np.testing.assert_array_equal(d2, _brute_d2(_queries(locref, world["scan"], pose), world["map"]))
        _check(gpu_ctx.icp_fitness(world["scan"], pose, 1.0), want)
        for rng in (0.3, 2.5):
            _check(gpu_ctx.icp_fitness(world["scan"], pose, rng), _expected(locref, world["tree"], world["map"], world["scan"], pose, rng, clear_of_gate=False)[0])


def test_fitness_is_the_exact_neighbour_not_the_pruned_one(gpu_ctx, locref, world):
    """The alpha = 0.1 walk of the matcher's defaults returns a farther point for a good share of the queries; the score must not."""
    q = _queries(locref, world["scan"], world["init"])
    approx = _d2(q, world["map"][world["tree"].knn(q, k=1, approximate=True, alpha=0.1)[:, 0]])
    exact = _d2(q, world["map"][world["tree"].knn(q, k=1, approximate=False)[:, 0]])
    assert (approx > exact).mean() > 0.02  # the distinction is real on these inputs
    got = gpu_ctx.icp_fitness(world["scan"], world["init"], float("inf"))
    assert abs(got["score"] - float(exact.astype(np.float64).mean())) <= SUM_RTOL * got["score"]


def test_fitness_infinite_range_counts_every_finite_point(gpu_ctx, locref, world):
    want, _ = _expected(locref, world["tree"], world["map"], world["scan"], world["init"], float("inf"))
    assert want["inliers"] == want["finite_points"] == 4000
    _check(gpu_ctx.icp_fitness(world["scan"], world["init"], float("inf")), want)


def test_fitness_skips_non_finite_points(gpu_ctx, locref, world):
    s = np.array(world["scan"], copy=True)
    s[5, 0] = np.nan
    s[77, 2] = np.inf
    s[1234, 1] = -np.inf
    s[3999] = np.nan
    want, _ = _expected(locref, world["tree"], world["map"], s, world["true"], 1.0)
    assert want["finite_points"] == 3996
    _check(gpu_ctx.icp_fitness(s, world["true"], 1.0), want)


def test_fitness_far_away_has_no_inlier(gpu_ctx, world):
    far = world["true"].copy()
    far[4] += 1000.0
    got = gpu_ctx.icp_fitness(world["scan"], far, 1.0)
    assert got == dict(score=float("inf"), inliers=0, finite_points=4000)


def test_fitness_is_deterministic_and_independent_of_batching(api, gpu_ctx, synth, world):
    s = world["scan"]
    poses = np.array([world["true"], world["init"], _more_poses(synth, world["true"])[0]])
    one = [bytes(gpu_ctx.icp_fitness(s, p, 1.0, raw=True)) for p in poses]
    assert one == [bytes(gpu_ctx.icp_fitness(s, p, 1.0, raw=True)) for p in poses]  # two calls: identical bytes
    assert bytes(gpu_ctx.icp_fitness(s, poses, 1.0, raw=True)) == b"".join(one)  # three poses in one call = three calls
    # an ordinary 4-scan batch (scans of different lengths) = four single calls
    scans = [s, s[:2500], s[1000:], s[::3]]
    bp = np.array([poses[0], poses[1], poses[2], poses[1]])
    b = gpu_ctx.batch(scans)
    try:
        got = bytes(gpu_ctx.icp_fitness_batch(b, bp, 1.0, raw=True))
        assert got == b"".join(bytes(gpu_ctx.icp_fitness(sc, p, 1.0, raw=True)) for sc, p in zip(scans, bp))
        assert got == bytes(gpu_ctx.icp_fitness_batch(b, bp, 1.0, raw=True))
    finally:
        b.close()
    # a shared-source batch = the batch of uploaded copies
    sh, cp = gpu_ctx.batch_shared(s, 3), gpu_ctx.batch([s, s, s])
    try:
        assert bytes(gpu_ctx.icp_fitness_batch(sh, poses, 1.0, raw=True)) == bytes(gpu_ctx.icp_fitness_batch(cp, poses, 1.0, raw=True)) == b"".join(one)
    finally:
        sh.close()
        cp.close()


def test_fitness_leaves_alignments_alone(api, gpu_ctx, world):
    """A score between two alignments changes nothing about them (it shares the one-scan batch and its work lists)."""
    opts = api.icp_opts(method=api.P2PLANE)
    a, sa = gpu_ctx.icp_align(world["scan"], world["init"], opts)
    gpu_ctx.icp_fitness(world["scan"], a, 1.0)
    b, sb = gpu_ctx.icp_align(world["scan"], world["init"], opts)
    assert a.tobytes() == b.tobytes() and sa == sb
    # ... and the resident form scores the cloud the alignment left in HBM
    assert gpu_ctx.icp_fitness_resident(b, 1.0) == gpu_ctx.icp_fitness(world["scan"], b, 1.0)


def test_fitness_argument_errors(api, gpu_ctx, world):
    s, p = world["scan"], world["true"]
    fresh = api.Context(0)
    try:
        with pytest.raises(api.LocGpuError) as e:
            fresh.icp_fitness(s, p, 1.0)
        assert e.value.code == -3  # LOCGPU_ERR_NO_TARGET
        with pytest.raises(api.LocGpuError) as e:
            fresh.icp_init_search(s, p, api.icp_opts())
        assert e.value.code == -3
    finally:
        fresh.close()
    for bad in (lambda: gpu_ctx.icp_fitness(s, p, float("nan")), lambda: gpu_ctx.icp_fitness(s[:0], p, 1.0),
                lambda: gpu_ctx.icp_fitness(s, np.zeros((0, 7)), 1.0),
                lambda: gpu_ctx.icp_init_search(s, np.zeros((0, 7)), api.icp_opts()),
                lambda: gpu_ctx.icp_init_search(s[:0], p, api.icp_opts()),
                lambda: gpu_ctx.icp_init_search(s, p, api.icp_opts(), api.init_search_opts(max_range=float("nan"))),
                lambda: gpu_ctx.icp_init_search(s, p, api.icp_opts(), api.init_search_opts(min_inlier_ratio=-0.1))):
        with pytest.raises(api.LocGpuError) as e:
            bad()
        assert e.value.code == -1  # LOCGPU_ERR_INVALID
    sh = gpu_ctx.batch_shared(s, 2)
    try:
        with pytest.raises(api.LocGpuError) as e:
            sh.upload_async([s, s])
        assert e.value.code == -1
    finally:
        sh.close()


def test_fitness_full_size(api, synth, locref):
    """One 115 200-point scan against the 10 M-point map, against the oracle's exact list."""
    m = synth.make_map(10_000_000)
    s = synth.make_scan(0)
    assert len(s) == 115200
    true_pose, init_pose = synth.make_pose(0)
    tree = locref.KdTree(m)
    ctx = api.Context(0)
    try:
        ctx.icp_set_target(m)
        mx = np.ascontiguousarray(m[:, :3])
        for pose in (true_pose, init_pose):
            _check(ctx.icp_fitness(s, pose, 1.0), _expected(locref, tree, mx, s, pose, 1.0)[0])
        assert bytes(ctx.icp_fitness(s, np.array([true_pose, init_pose]), 1.0, raw=True)) == \
            bytes(ctx.icp_fitness(s, true_pose, 1.0, raw=True)) + bytes(ctx.icp_fitness(s, init_pose, 1.0, raw=True))
    finally:
        ctx.close()
