"""The NDT fitness score (include/locgpu.h: locgpu_ndt_fitness, _batch, _resident) against its definition restated with numpy from the
ORACLE's voxel table and the oracle's transform (tests/ndt_score_ref.py): counts equal, the FP64 sum within 1e-9 relative (the
project's bar for FP64 sums whose order differs)."""
import numpy as np
import pytest

import ndt_score_ref as ref

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-9
GATE_MARGIN = 1e-9  # no (point, voxel) residual of the inputs lies this close to res_outlier_th: the counts are unambiguous
RES_TH = 20.0       # NdtOptions::res_outlier_th_ default
CENTER, NEARBY6 = 0, 1


@pytest.fixture(scope="module")
def world(synth, locref):
    m = synth.make_local_map(200_000, 7, half=40)
    s = synth.make_scan(7, crop_half=30, subsample=4000)
    assert len(s) == 4000
    true_pose, init_pose = synth.make_pose(7)
    ndt = locref.Ndt()  # the table does not depend on the nearby type
    ndt.set_target(m)
    return dict(map=m, scan=s, true=true_pose, init=init_pose, table=ref.Table(*ndt.dump()))


def _more_poses(synth, true_pose):
    a = true_pose.copy(); a[4:] += [0.7, -0.4, 0.05]
    _, b = synth.make_pose(7, trans_amp=1.0, rot_amp_deg=5.0)
    return [a, b]


def _target(api, ctx, world, nearby=NEARBY6):
    ctx.ndt_set_target(world["map"], api.ndt_opts(nearby_type=nearby))


def _expected(locref, world, scan, pose, n_nearby):
    res = ref.residuals(locref, world["table"], scan, pose, 1.0, n_nearby)
    margin = ref.gate_margin(res, RES_TH)
    assert margin > GATE_MARGIN, margin  # a condition on the inputs, checked on the CPU — not a tolerance on the kernel
    return ref.score_from_residuals(res, RES_TH, len(res))


def _check(got, want):
    print("ndt fitness: got %r want %r rel %.3e" % (got, want, abs(got["score"] - want["score"]) / want["score"] if np.isfinite(want["score"]) else 0.0))
    assert got["inliers"] == want["inliers"] and got["finite_points"] == want["finite_points"], (got, want)
    if np.isfinite(want["score"]):
        assert abs(got["score"] - want["score"]) <= SUM_RTOL * want["score"], (got, want)
    else:
        assert got["score"] == float("inf")


@pytest.mark.parametrize("nearby", [NEARBY6, CENTER])
def test_ndt_fitness_matches_definition(api, gpu_ctx, locref, synth, world, nearby):
    _target(api, gpu_ctx, world, nearby)
    n_nearby = 7 if nearby == NEARBY6 else 1
    wants = []
    for pose in [world["true"], world["init"]] + _more_poses(synth, world["true"]):
        want = _expected(locref, world, world["scan"], pose, n_nearby)
        assert 0 < want["inliers"] < 4000  # some points are gated or find no voxel: both branches of the count are exercised
        _check(gpu_ctx.ndt_fitness(world["scan"], pose), want)
        wants.append(want)
    assert wants[0]["score"] < wants[1]["score"] and wants[0]["inliers"] > wants[1]["inliers"]  # the true pose explains the scan better than the perturbed one


def test_ndt_fitness_skips_non_finite_points(api, gpu_ctx, locref, world):
    _target(api, gpu_ctx, world)
    s = np.array(world["scan"], copy=True)
    s[5, 0] = np.nan
    s[77, 2] = np.inf
    s[1234, 1] = -np.inf
    s[3999] = np.nan
    want = _expected(locref, world, s, world["true"], 7)
    assert want["finite_points"] == 3996
    _check(gpu_ctx.ndt_fitness(s, world["true"]), want)


def test_ndt_fitness_far_away_has_no_inlier(api, gpu_ctx, world):
    _target(api, gpu_ctx, world)
    far = world["true"].copy()
    far[4] += 1000.0
    assert gpu_ctx.ndt_fitness(world["scan"], far) == dict(score=float("inf"), inliers=0, finite_points=4000)


def test_ndt_fitness_is_deterministic_and_independent_of_batching(api, gpu_ctx, synth, world):
    _target(api, gpu_ctx, world)
    s = world["scan"]
    poses = np.array([world["true"], world["init"], _more_poses(synth, world["true"])[0]])
    one = [bytes(gpu_ctx.ndt_fitness(s, p, raw=True)) for p in poses]
    assert one == [bytes(gpu_ctx.ndt_fitness(s, p, raw=True)) for p in poses]  # two runs: identical bytes
    assert bytes(gpu_ctx.ndt_fitness(s, poses, raw=True)) == b"".join(one)  # alone = among three poses
    # ordinary batches of 1, 3 and 5 scans (of different lengths) = single calls
    scans = [s, s[:2500], s[1000:], s[::3], s[:1025]]
    bp = np.array([poses[0], poses[1], poses[2], poses[1], poses[0]])
    single = [bytes(gpu_ctx.ndt_fitness(sc, p, raw=True)) for sc, p in zip(scans, bp)]
    assert single[0] == one[0]
    for k in (1, 3, 5):
        b = gpu_ctx.batch(scans[:k])
        try:
            got = bytes(gpu_ctx.ndt_fitness_batch(b, bp[:k], raw=True))
            assert got == b"".join(single[:k]), k
            assert got == bytes(gpu_ctx.ndt_fitness_batch(b, bp[:k], raw=True))
        finally:
            b.close()
    # a shared-source batch = the batch of uploaded copies = single calls
    sh, cp = gpu_ctx.batch_shared(s, 3), gpu_ctx.batch([s, s, s])
    try:
        assert bytes(gpu_ctx.ndt_fitness_batch(sh, poses, raw=True)) == bytes(gpu_ctx.ndt_fitness_batch(cp, poses, raw=True)) == b"".join(one)
    finally:
        sh.close()
        cp.close()


def test_ndt_fitness_resident_scores_the_cloud_the_alignment_left(api, gpu_ctx, world):
    _target(api, gpu_ctx, world)
    a, sa = gpu_ctx.ndt_align(world["scan"], world["init"])
    resident = gpu_ctx.ndt_fitness_resident(a)
    assert resident == gpu_ctx.ndt_fitness(world["scan"], a)  # equal floats: the same bits (no NaN here)
    assert np.isfinite(resident["score"]) and resident["finite_points"] == 4000
    # a score between two alignments changes nothing about them
    b, sb = gpu_ctx.ndt_align(world["scan"], world["init"])
    assert a.tobytes() == b.tobytes() and sa == sb
    # ... and ScanMatch leaves the same copy behind
    pose, _, _ = gpu_ctx.ndt_scan_match(world["scan"], world["init"])[:3]
    assert gpu_ctx.ndt_fitness_resident(pose) == gpu_ctx.ndt_fitness(world["scan"], pose)


def test_ndt_fitness_argument_errors(api, world):
    s, p = world["scan"], world["true"]
    fresh = api.Context(0)
    try:
        for call in (lambda: fresh.ndt_fitness(s, p), lambda: fresh.ndt_fitness_resident(p), lambda: fresh.ndt_init_search(s, p)):
            with pytest.raises(api.LocGpuError) as e:
                call()
            assert e.value.code == -3  # LOCGPU_ERR_NO_TARGET
        fresh.ndt_set_target(world["map"])
        for bad in (lambda: fresh.ndt_fitness(s[:0], p), lambda: fresh.ndt_fitness(s, np.zeros((0, 7))), lambda: fresh.ndt_init_search(s, np.zeros((0, 7))),
                    lambda: fresh.ndt_init_search(s[:0], p), lambda: fresh.ndt_init_search(s, p, api.init_search_opts(min_inlier_ratio=-0.1)),
                    lambda: fresh.ndt_init_search(s, p, api.init_search_opts(min_inlier_ratio=float("nan"))),
                    lambda: fresh.ndt_fitness_resident(p)):  # no single-scan call has left a cloud yet
            with pytest.raises(api.LocGpuError) as e:
                bad()
            assert e.value.code == -1  # LOCGPU_ERR_INVALID
        # sopts->max_range is not used: a NaN there is not an error
        assert fresh.ndt_init_search(s, p, api.init_search_opts(max_range=float("nan")))[3] in (0, -1)
        # the incremental target is refused, in words
        fresh.ndt_set_target(world["map"], api.ndt_opts(method=2, capacity=100000))
        b = fresh.batch([s])
        try:
            for call in (lambda: fresh.ndt_fitness(s, p), lambda: fresh.ndt_fitness_batch(b, p), lambda: fresh.ndt_fitness_resident(p),
                         lambda: fresh.ndt_init_search(s, p)):
                with pytest.raises(api.LocGpuError) as e:
                    call()
                assert e.value.code == -1 and "incremental" in str(e.value)
        finally:
            b.close()
    finally:
        fresh.close()
