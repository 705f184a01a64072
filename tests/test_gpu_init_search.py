"""Shared-source batches and the initial-pose search (include/locgpu.h: locgpu_batch_create_shared, locgpu_icp_init_search), and the
façade's GetFitnessScore / InitialPoseSearch. Expected values come from the oracle and numpy, never from the library."""
import os
import subprocess

import numpy as np
import pytest

from conftest import pose_delta

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4    # the project's pose bar
POSE_TOL_RAD = 1e-4
SUM_RTOL = 1e-9


def _np_fitness(locref, tree, map_xyz, scan, pose, max_range):
    q = locref.transform_points(pose, np.ascontiguousarray(scan[:, :3], dtype=np.float64)).astype(np.float32)
    d = q - map_xyz[tree.knn(q, k=1, approximate=False)[:, 0]]
    d2 = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    inl = d2 <= np.float32(max_range * max_range)
    n = int(inl.sum())
    return dict(score=float(d2[inl].astype(np.float64).sum() / n) if n else float("inf"), inliers=n, finite_points=len(q))


def _fit_list(raw):
    return [dict(score=f.score, inliers=int(f.inliers), finite_points=int(f.finite_points)) for f in raw]


@pytest.fixture(scope="module")
def scan(synth):
    s = synth.make_scan(7, crop_half=30, subsample=4000)
    assert len(s) == 4000
    return s


@pytest.fixture(scope="module")
def centre(synth):
    """The true pose turned by 0.08 rad about z and moved by (1.3, -0.9, 0) m."""
    true_pose, _ = synth.make_pose(7)
    x, y, z, w = true_pose[:4]
    s, c = np.sin(0.04), np.cos(0.04)
    q = np.array([w * 0 + x * c + y * s, -x * s + y * c, w * s + z * c, w * c - z * s])  # true ⊗ rot_z(0.08)
    return np.concatenate([q, true_pose[4:] + [1.3, -0.9, 0.0]])


# ------------------------------------------------------------------------------------------------ shared-source batch
@pytest.fixture(scope="module")
def small_target(synth, gpu_ctx):
    m = synth.make_local_map(200_000, 7, half=40)
    gpu_ctx.icp_set_target(m)
    return m


def _reference_batch(api, gpu_ctx, s, cands, opts, max_range):
    """The ordinary batch that holds one uploaded copy of the scan per candidate."""
    b = gpu_ctx.batch([s] * len(cands))
    try:
        poses, stats = gpu_ctx.icp_align_batch(b, cands, opts)
        fit = bytes(gpu_ctx.icp_fitness_batch(b, poses, max_range, raw=True))
    finally:
        b.close()
    return poses, stats, fit


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("method", [0, 1, 2])
def test_shared_source_equals_uploaded_copies(api, gpu_ctx, small_target, scan, centre, method, graph):
    cands, n = api.pose_grid(centre, 1.0, 1.0, 0.1, 0.1)
    assert n == 27
    opts = api.icp_opts(method=method)
    gpu_ctx.graph_enable(graph)
    try:
        want_poses, want_stats, want_fit = _reference_batch(api, gpu_ctx, scan, cands, opts, 1.0)
        poses, fit, stats, best = gpu_ctx.icp_init_search(scan, cands, opts, raw=True)
        assert poses.tobytes() == want_poses.tobytes() and stats == want_stats and bytes(fit) == want_fit
        # the batch itself, through the ordinary batch entry points
        sh = gpu_ctx.batch_shared(scan, len(cands))
        try:
            p2, s2 = gpu_ctx.icp_align_batch(sh, cands, opts)
            assert p2.tobytes() == want_poses.tobytes() and s2 == want_stats
            assert bytes(gpu_ctx.icp_fitness_batch(sh, p2, 1.0, raw=True)) == want_fit
            gpu_ctx.icp_align_batch_begin(sh, cands, opts)
            p3, s3 = gpu_ctx.align_batch_end(sh)
            assert p3.tobytes() == want_poses.tobytes() and s3 == want_stats
            hb = gpu_ctx.icp_hb_batch(sh, cands, opts)
        finally:
            sh.close()
        cp = gpu_ctx.batch([scan] * len(cands))
        try:
            assert hb.tobytes() == gpu_ctx.icp_hb_batch(cp, cands, opts).tobytes()
        finally:
            cp.close()
        # the winner is the rule of the header applied to the reported scores
        f = _fit_list(fit)
        ok = [i for i in range(len(f)) if f[i]["inliers"] >= 1 and f[i]["inliers"] >= 0.5 * f[i]["finite_points"]]
        assert best == (min(ok, key=lambda i: (f[i]["score"], i)) if ok else -1)
    finally:
        gpu_ctx.graph_enable(False)


@pytest.mark.parametrize("method,graph,grid", [(2, False, False), (0, True, False), (2, False, True)])
def test_shared_source_in_chunks_equals_uploaded_copies(api, gpu_ctx, small_target, scan, centre, method, graph, grid):
    """325 candidates of a 4 000-point scan: more than one chunk holds (256), so two run — and nothing of that shows."""
    cands, n = api.pose_grid(centre, 2.0, 1.0, 0.3, 0.05)
    assert n == 325 and n > 256
    opts = api.icp_opts(method=method, search_mode=api.SEARCH_GRID_EXACT if grid else api.SEARCH_TREE_FAITHFUL)
    gpu_ctx.graph_enable(graph)
    try:
        want_poses, want_stats, want_fit = _reference_batch(api, gpu_ctx, scan, cands, opts, 1.0)
        poses, fit, stats, best = gpu_ctx.icp_init_search(scan, cands, opts, raw=True)
        assert poses.tobytes() == want_poses.tobytes() and stats == want_stats and bytes(fit) == want_fit
        # a second call reuses the context's workspace; a shorter one fits inside it
        poses2, fit2, stats2, best2 = gpu_ctx.icp_init_search(scan, cands, opts, raw=True)
        assert poses2.tobytes() == poses.tobytes() and bytes(fit2) == bytes(fit) and stats2 == stats and best2 == best
        p3, f3, s3, _ = gpu_ctx.icp_init_search(scan[:3000], cands[:5], opts, raw=True)
        w3 = _reference_batch(api, gpu_ctx, scan[:3000], cands[:5], opts, 1.0)
        assert p3.tobytes() == w3[0].tobytes() and s3 == w3[1] and bytes(f3) == w3[2]
    finally:
        gpu_ctx.graph_enable(False)


def test_init_search_single_candidate_and_no_winner(api, gpu_ctx, small_target, scan, synth):
    _, init = synth.make_pose(7)
    opts = api.icp_opts(method=api.P2PLANE)
    want_pose, want_stats = gpu_ctx.icp_align(scan, init, opts)
    want_fit = bytes(gpu_ctx.icp_fitness(scan, want_pose, 1.0, raw=True))
    poses, fit, stats, best = gpu_ctx.icp_init_search(scan, init, opts, raw=True)
    assert poses[0].tobytes() == want_pose.tobytes() and stats[0] == want_stats and bytes(fit) == want_fit and best == 0
    # nobody reaches an inlier ratio of 1.1: no winner, every output still filled
    cands, _ = api.pose_grid(init, 1.0, 1.0, 0.0, 0.0)
    ref = gpu_ctx.icp_init_search(scan, cands, opts, raw=True)
    poses, fit, stats, best = gpu_ctx.icp_init_search(scan, cands, opts, api.init_search_opts(min_inlier_ratio=1.1), raw=True)
    assert best == -1 and ref[3] >= 0
    assert poses.tobytes() == ref[0].tobytes() and bytes(fit) == bytes(ref[1]) and stats == ref[2]
    assert all(s["iterations"] > 0 for s in stats) and all(f.finite_points == 4000 for f in fit)


# ------------------------------------------------------------------------------------------------ the search against the oracle
def test_init_search_finds_the_oracles_winner(api, gpu_ctx, locref, synth, scan, centre):
    m = synth.make_local_map(1_000_000, 7, half=40)
    mx = np.ascontiguousarray(m[:, :3])
    true_pose, _ = synth.make_pose(7)
    cands, n = api.pose_grid(centre, 2.0, 1.0, 0.15, 0.05)
    assert n == 175
    # ---- the CPU side alone: the reference's loop from every candidate, every result scored with numpy
    icp = locref.Icp(method=locref.P2PLANE)
    icp.set_target(m)
    tree = locref.KdTree(m)
    cpu = [icp.align(scan, c) for c in cands]
    cpu_fit = [_np_fitness(locref, tree, mx, scan, r["pose"], 1.0) for r in cpu]
    score = np.array([f["score"] for f in cpu_fit])
    order = np.argsort(score, kind="stable")
    win = int(order[0])
    ratios = np.array([f["inliers"] / f["finite_points"] for f in cpu_fit])
    print("CPU: winner %d score %.6f (%d iterations, %.4f m from the true pose), runner-up %.6f, inlier ratios >= %.3f, capped runs %d"
          % (win, score[win], cpu[win]["iters"], pose_delta(cpu[win]["pose"], true_pose)[0], score[order[1]], ratios.min(),
             sum(r["iters"] >= 20 for r in cpu)))
    assert pose_delta(cpu[win]["pose"], true_pose)[0] <= 0.1
    assert score[order[1]] >= 1.01 * score[win]
    assert ratios.min() >= 0.5
    # ---- the GPU
    gpu_ctx.icp_set_target(m)
    opts = api.icp_opts(method=api.P2PLANE)
    poses, fit, stats, best = gpu_ctx.icp_init_search(scan, cands, opts, api.init_search_opts(max_range=1.0))
    assert best == win
    dt, dr = pose_delta(poses[best], cpu[win]["pose"])
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (dt, dr)
    assert pose_delta(poses[best], true_pose)[0] <= 0.1
    # the score everywhere, at the GPU's own poses: no alignment difference is inherited
    for i in range(n):
        want = _np_fitness(locref, tree, mx, scan, poses[i], 1.0)
        assert fit[i]["inliers"] == want["inliers"] and fit[i]["finite_points"] == want["finite_points"], (i, fit[i], want)
        assert abs(fit[i]["score"] - want["score"]) <= SUM_RTOL * want["score"], (i, fit[i], want)
    # the alignment, where the oracle's run left through |dx| < eps before the cap
    worst_capped = (0.0, 0.0)
    for i in range(n):
        dt, dr = pose_delta(poses[i], cpu[i]["pose"])
        if cpu[i]["iters"] < 20:
            assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (i, dt, dr)
            assert stats[i]["iterations"] == cpu[i]["iters"], (i, stats[i], cpu[i]["iters"])
        else:
            worst_capped = (max(worst_capped[0], dt), max(worst_capped[1], dr))
    print("capped runs (20 iterations, no bar set): largest pose difference to the oracle %.3e m / %.3e rad" % worst_capped)


# ------------------------------------------------------------------------------------------------ façade
@pytest.mark.parametrize("method", [2, 0])
def test_cpp_facade_fitness_and_initial_pose_search(api, locref, synth, scan, centre, tmp_path, method):
    """IcpRegistration::EnableFitnessScore / GetFitnessScore / InitialPoseSearch (tests/cpp/facade_fitness.cpp): 0.0f without the
    opt-in, ScanMatch byte-identical with and without it, the score that of locgpu_icp_fitness at the result pose, the search what
    locgpu_icp_init_search returns — the driver compares those bit for bit; the values themselves are checked here."""
    exe = os.path.join(os.path.dirname(__file__), "cpp", "facade_fitness")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    m = synth.make_local_map(200_000, 7, half=40)
    _, init = synth.make_pose(7)
    cands, _ = api.pose_grid(centre, 1.0, 1.0, 0.1, 0.1)
    np.ascontiguousarray(m[:, :3], dtype=np.float32).tofile(tmp_path / "map.bin")
    np.ascontiguousarray(scan[:, :3], dtype=np.float32).tofile(tmp_path / "scan.bin")
    np.asarray(init, dtype=np.float64).tofile(tmp_path / "pose.bin")
    np.ascontiguousarray(cands, dtype=np.float64).tofile(tmp_path / "cands.bin")
    r = subprocess.run([exe, str(method), str(tmp_path / "map.bin"), str(tmp_path / "scan.bin"), str(tmp_path / "pose.bin"), str(tmp_path / "cands.bin"),
                        str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    out = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    pose, facade_score, abi_score, inliers, finite = out[:7], out[7], out[8], int(out[9]), int(out[10])
    best_pose, best_score, best = out[11:18], out[18], int(out[19])
    want = _np_fitness(locref, locref.KdTree(m), np.ascontiguousarray(m[:, :3]), scan, pose, 1.0)
    assert (inliers, finite) == (want["inliers"], want["finite_points"])
    assert abs(abi_score - want["score"]) <= SUM_RTOL * want["score"]
    assert np.float32(facade_score) == np.float32(abi_score) and facade_score > 0
    assert 0 <= best < len(cands)
    bw = _np_fitness(locref, locref.KdTree(m), np.ascontiguousarray(m[:, :3]), scan, best_pose, 1.0)
    assert abs(best_score - bw["score"]) <= 1e-6 * bw["score"]  # a float32 in the façade's interface
