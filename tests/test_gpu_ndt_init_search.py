"""The initial-pose search with the NDT matcher (include/locgpu.h: locgpu_ndt_init_search) and the façade's
NdtRegistration::EnableFitnessScore / GetFitnessScore / InitialPoseSearch. Expected values come from the oracle and from the numpy
restatement of the score (tests/ndt_score_ref.py), never from the library."""
import os
import subprocess

import numpy as np
import pytest

import ndt_score_ref as ref
from conftest import pose_delta

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4    # the project's pose bar
POSE_TOL_RAD = 1e-4
SUM_RTOL = 1e-9
WINNER_MARGIN = 1e-6  # runner-up over winner, relative: 1000 × the sum bar, so the order of a sum cannot flip the winner
MAX_ITERATION = 20


@pytest.fixture(scope="module")
def world(synth, locref):
    m = synth.make_local_map(200_000, 7, half=40)
    s = synth.make_scan(7, crop_half=30, subsample=4000)
    assert len(s) == 4000
    true_pose, init_pose = synth.make_pose(7)
    ndt = locref.Ndt()
    ndt.set_target(m)
    # the true pose turned by 0.08 rad about z and moved by (1.3, -0.9, 0) m: the centre test_gpu_init_search.py searches around
    x, y, z, w = true_pose[:4]
    sn, c = np.sin(0.04), np.cos(0.04)
    q = np.array([x * c + y * sn, -x * sn + y * c, w * sn + z * c, w * c - z * sn])
    centre = np.concatenate([q, true_pose[4:] + [1.3, -0.9, 0.0]])
    return dict(map=m, scan=s, true=true_pose, init=init_pose, ndt=ndt, table=ref.Table(*ndt.dump()), centre=centre)


@pytest.fixture(scope="module")
def cands(api, world):
    c, n = api.pose_grid(world["centre"], 2.0, 1.0, 0.3, 0.05)
    assert n == 325 and n > 256  # more than one chunk holds: two run
    return c


def _oracle_aligns(locref, m, s, cands, workers=8):
    """The oracle's loop from every candidate, on a few threads (one oracle object each; the calls release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor

    def run(part):
        ndt = locref.Ndt()
        ndt.set_target(m)
        return [ndt.align(s, c) for c in part]

    parts = [cands[i::workers] for i in range(workers)]
    with ThreadPoolExecutor(workers) as ex:
        done = list(ex.map(run, parts))
    out = [None] * len(cands)
    for i, part in enumerate(done):
        out[i::workers] = part
    return out


def _fit_list(raw):
    return [dict(score=f.score, inliers=int(f.inliers), finite_points=int(f.finite_points)) for f in raw]


@pytest.mark.parametrize("graph", [False, True])
def test_ndt_init_search_equals_the_shared_batch_bit_for_bit(api, gpu_ctx, world, cands, graph):
    gpu_ctx.ndt_set_target(world["map"])
    s = world["scan"]
    gpu_ctx.graph_enable(graph)
    try:
        sh = gpu_ctx.batch_shared(s, len(cands))
        try:
            want_poses, want_stats = gpu_ctx.ndt_align_batch(sh, cands)
            want_fit = bytes(gpu_ctx.ndt_fitness_batch(sh, want_poses, raw=True))
        finally:
            sh.close()
        poses, fit, stats, best = gpu_ctx.ndt_init_search(s, cands, raw=True)
        assert poses.tobytes() == want_poses.tobytes() and stats == want_stats and bytes(fit) == want_fit
        assert best == ref.winner(_fit_list(fit)) and best >= 0
        # a second call reuses the context's workspace; a shorter one fits inside it
        poses2, fit2, stats2, best2 = gpu_ctx.ndt_init_search(s, cands, raw=True)
        assert poses2.tobytes() == poses.tobytes() and bytes(fit2) == bytes(fit) and stats2 == stats and best2 == best
        p3, f3, s3, _ = gpu_ctx.ndt_init_search(s[:3000], cands[:5], raw=True)
        cp = gpu_ctx.batch([s[:3000]] * 5)
        try:
            w3, ws3 = gpu_ctx.ndt_align_batch(cp, cands[:5])
            assert p3.tobytes() == w3.tobytes() and s3 == ws3 and bytes(f3) == bytes(gpu_ctx.ndt_fitness_batch(cp, w3, raw=True))
        finally:
            cp.close()
        # nobody reaches an inlier ratio of 1.1: no winner, every output still filled
        p4, f4, s4, b4 = gpu_ctx.ndt_init_search(s, cands[:7], api.init_search_opts(min_inlier_ratio=1.1), raw=True)
        assert b4 == -1 and all(f.finite_points == 4000 for f in f4) and all(x["iterations"] > 0 for x in s4)
    finally:
        gpu_ctx.graph_enable(False)


def test_ndt_init_search_against_the_oracle(api, gpu_ctx, locref, world, cands):
    """On this world NDT's score does NOT single out a pose near the true one: the oracle's loop from these candidates
    mostly ends at the iteration cap or after one step, and the lowest mean χ² belongs to a candidate metres away that explains fewer
    points well. What holds, and is asserted: the GPU runs the oracle's loop from every candidate, scores as the definition says and
    picks the winner the definition picks at the oracle's poses."""
    s, n = world["scan"], len(cands)
    # ---- the CPU side alone: the reference's loop from every candidate, every result scored with the restatement
    cpu = _oracle_aligns(locref, world["map"], s, cands)
    cpu_fit = [ref.score(locref, world["table"], s, r["pose"]) for r in cpu]
    score = np.array([f["score"] for f in cpu_fit])
    order = np.argsort(score, kind="stable")
    win = ref.winner(cpu_fit)
    ratios = np.array([f["inliers"] / f["finite_points"] for f in cpu_fit])
    capped = sum(r["iters"] >= MAX_ITERATION for r in cpu)
    print("CPU: winner %d score %.9f (%d iterations, %.4f m from the true pose, inlier ratio %.4f), runner-up %d score %.9f, inlier ratios >= %.3f, "
          "capped runs %d, score at the true pose %.6f"
          % (win, score[win], cpu[win]["iters"], pose_delta(cpu[win]["pose"], world["true"])[0], ratios[win], order[1], score[order[1]], ratios.min(),
             capped, ref.score(locref, world["table"], s, world["true"])["score"]))
    assert win == int(order[0]) and ratios.min() >= 0.5  # every candidate qualifies: the winner is the plain minimum
    assert score[order[1]] >= (1.0 + WINNER_MARGIN) * score[win]  # a condition on the inputs, from the CPU alone
    assert all(r["status"] == 0 for r in cpu)
    # ---- the GPU
    gpu_ctx.ndt_set_target(world["map"])
    poses, fit, stats, best = gpu_ctx.ndt_init_search(s, cands)
    # the score everywhere, at the GPU's own poses: no alignment difference is inherited
    for i in range(n):
        want = ref.score(locref, world["table"], s, poses[i])
        assert fit[i]["inliers"] == want["inliers"] and fit[i]["finite_points"] == want["finite_points"], (i, fit[i], want)
        assert abs(fit[i]["score"] - want["score"]) <= SUM_RTOL * want["score"], (i, fit[i], want)
    # the alignment, where the oracle's run left through |dx| < eps before the cap
    worst_capped = (0.0, 0.0)
    for i in range(n):
        dt, dr = pose_delta(poses[i], cpu[i]["pose"])
        if cpu[i]["iters"] < MAX_ITERATION:
            assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (i, dt, dr)
            assert stats[i]["iterations"] == cpu[i]["iters"], (i, stats[i], cpu[i]["iters"])
        else:
            worst_capped = (max(worst_capped[0], dt), max(worst_capped[1], dr))
    print("capped runs (%d iterations, no bar set): largest pose difference to the oracle %.3e m / %.3e rad" % ((MAX_ITERATION,) + worst_capped))
    assert best == win


def test_cpp_facade_ndt_fitness_and_initial_pose_search(api, locref, world, tmp_path):
    """NdtRegistration::EnableFitnessScore / GetFitnessScore / InitialPoseSearch (tests/cpp/facade_ndt_fitness.cpp): 0.0f without the
    opt-in, ScanMatch byte-identical with and without it, the score that of locgpu_ndt_fitness at the result pose, the search what
    locgpu_ndt_init_search returns, the incremental method refused — the driver compares those bit for bit; the values are checked here."""
    exe = os.path.join(os.path.dirname(__file__), "cpp", "facade_ndt_fitness")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    m, s = world["map"], world["scan"]
    cands, n = api.pose_grid(world["centre"], 1.0, 1.0, 0.1, 0.1)
    assert n == 27
    np.ascontiguousarray(m[:, :3], dtype=np.float32).tofile(tmp_path / "map.bin")
    np.ascontiguousarray(s[:, :3], dtype=np.float32).tofile(tmp_path / "scan.bin")
    np.asarray(world["init"], dtype=np.float64).tofile(tmp_path / "pose.bin")
    np.ascontiguousarray(cands, dtype=np.float64).tofile(tmp_path / "cands.bin")
    r = subprocess.run([exe, str(tmp_path / "map.bin"), str(tmp_path / "scan.bin"), str(tmp_path / "pose.bin"), str(tmp_path / "cands.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    out = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    pose, facade_score, abi_score, inliers, finite = out[:7], out[7], out[8], int(out[9]), int(out[10])
    best_pose, best_score, best = out[11:18], out[18], int(out[19])
    want = ref.score(locref, world["table"], s, pose)
    assert (inliers, finite) == (want["inliers"], want["finite_points"])
    assert abs(abi_score - want["score"]) <= SUM_RTOL * want["score"]
    assert np.float32(facade_score) == np.float32(abi_score) and facade_score > 0
    assert 0 <= best < len(cands)
    bw = ref.score(locref, world["table"], s, best_pose)
    assert abs(best_score - bw["score"]) <= 1e-6 * bw["score"]  # a float32 in the façade's interface
