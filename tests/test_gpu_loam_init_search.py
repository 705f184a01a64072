"""The LOAM matcher's joint fitness score and batched initial-pose search (include/locgpu.h: locgpu_loam_fitness[_cloud],
locgpu_loam_init_search[_cloud], locgpu_loam_create_on) and the façade's LoamRegistration::GetFitnessScore / InitialPoseSearch.
Expected values come from the oracle composition of tests/loam_ref.py and the numpy score of tests/loam_score_ref.py, or from the
library's own older entry points (locgpu_loam_align_batch, locgpu_icp_fitness) where the claim is bit-identity.

The world is the small world's split, cut to the sizes at which the code can still go wrong: an edge scan of 715 points (one
1 024-point fitness row, which is also the last), a surface scan of 2 500 (three rows, the last partial); 7 candidates (one chunk, odd,
below a wave) and 260 (two equal chunks of 130, as a chunk holds at most 256). LoamOption's eps = 1e-3 does not converge within
20 iterations on this world, so the handle runs with eps = 1e-2, ICP's: the oracle alone then leaves all 7 candidates'
loops before the cap (17, 15, 6, 8, 13, 17, 6 iterations; DESIGN.md §14 records the CPU run)."""
import os
import subprocess

import numpy as np
import pytest

import loam_ref
import loam_score_ref as ref
from conftest import pose_delta

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4    # the project's pose bar
POSE_TOL_RAD = 1e-4
SUM_RTOL = 1e-9      # the bar DESIGN.md §9 sets for the same sums
EPS = 1e-2
MAX_RANGE = 1.0
FIT = np.dtype([("score", "f8"), ("inliers", "i8"), ("finite_points", "i8")])
# (rotation vector, translation) updates of the initial pose: the 7 candidates
OFFSETS = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0.004, 0.03, -0.02, 0], [0.003, -0.002, 0, -0.05, 0.04, 0.02], [0, 0, -0.006, 0.06, 0.05, 0],
                    [0, 0, 0.01, -0.08, 0.0, 0.0], [0.002, 0.002, 0.008, 0.1, -0.1, 0.01], [0, 0, -0.012, 0.0, 0.12, -0.02]])


def _fit(raw, m):
    """The ctypes array of 3 entries per candidate as a structured [m, 3] array: joint, surface, edge."""
    return np.frombuffer(bytes(raw), dtype=FIT).reshape(m, 3)


def _xyzi(a):
    out = np.zeros((len(a), 4), np.float32)
    out[:, :3] = a[:, :3]
    return out


def _as_dict(f):
    return dict(score=float(f["score"]), inliers=int(f["inliers"]), finite_points=int(f["finite_points"]))


@pytest.fixture(scope="module")
def world(small_world, locref):
    """The cut split, the candidates, the oracle's loop from each of the 7 and the numpy score at its poses — computed once, never modified."""
    w = loam_ref.split_world(small_world)
    w["edge"], w["surf"] = np.ascontiguousarray(w["edge"][::2]), np.ascontiguousarray(w["surf"][:2500])
    assert len(w["edge"]) == 715 and len(w["surf"]) == 2500
    w["cands7"] = np.array([locref.apply_update(w["init"], d) for d in OFFSETS])
    rng = np.random.default_rng(11)
    spread = rng.uniform(-1.0, 1.0, (260, 6)) * [0.004, 0.004, 0.012, 0.1, 0.1, 0.02]
    w["cands260"] = np.array([locref.apply_update(w["init"], d) for d in spread])
    w["cands260"][200] = w["cands7"][3]
    o = w["oracle"] = loam_ref.LoamOracle(locref, w["edge_map"], w["surf_map"])
    w["runs7"] = [o.scan_match(w["edge"], w["surf"], c, eps=EPS) for c in w["cands7"]]
    w["score"] = lambda pose, edge=w["edge"], surf=w["surf"]: ref.joint_score(w["edge_map"], w["surf_map"], edge, surf, pose, MAX_RANGE, locref.transform_points)
    w["fit7"] = [w["score"](r["pose"]) for r in w["runs7"]]
    return w


def _opts(api, grid=False, **kw):
    mode = api.SEARCH_GRID_EXACT if grid else api.SEARCH_TREE_FAITHFUL
    return api.loam_opts(eps=EPS, surf=api.icp_opts(method=api.P2PLANE, search_mode=mode), edge=api.icp_opts(method=api.P2LINE, search_mode=mode), **kw)


@pytest.fixture(scope="module")
def loam(api, world):
    h = api.Loam(_opts(api))
    h.set_target(world["edge_map"], world["surf_map"])
    yield h
    h.close()


@pytest.fixture(scope="module")
def plain(api, world):
    """Two plain ICP contexts holding the same maps: (surface, edge)."""
    s, e = api.Context(0), api.Context(0)
    s.icp_set_target(world["surf_map"])
    e.icp_set_target(world["edge_map"])
    yield s, e
    s.close()
    e.close()


@pytest.fixture(scope="module")
def search7(loam, world):
    return loam.init_search(world["edge"], world["surf"], world["cands7"], raw=True)


def _class_bits(plain, world, poses):
    """locgpu_icp_fitness of each class on its plain context under `poses`: ([m] surface, [m] edge) structured arrays."""
    s, e = plain
    return (np.frombuffer(bytes(s.icp_fitness(world["surf"], poses, MAX_RANGE, raw=True)), dtype=FIT),
            np.frombuffer(bytes(e.icp_fitness(world["edge"], poses, MAX_RANGE, raw=True)), dtype=FIT))


# ------------------------------------------------------------------------------------------------ 1. chunks never show
@pytest.mark.parametrize("grid", [False, True])
def test_search_in_two_chunks_equals_the_batch_of_copies(api, world, plain, grid):
    cands, m = world["cands260"], 260
    h = api.Loam(_opts(api, grid))
    try:
        h.set_target(world["edge_map"], world["surf_map"])
        want_poses, want_stats = h.align_batch([world["edge"]] * m, [world["surf"]] * m, cands)
        want_surf, want_edge = _class_bits(plain, world, want_poses)
        poses, fit, stats, best = h.init_search(world["edge"], world["surf"], cands, raw=True)
        f = _fit(fit, m)
        print("iterations", sorted(set(s["iterations"] for s in stats)), "best", best)
        assert poses.tobytes() == want_poses.tobytes() and stats == want_stats
        assert f[:, 1].tobytes() == want_surf.tobytes() and f[:, 2].tobytes() == want_edge.tobytes()
        # the resident form: the same bits, and so is a second call on the grown workspace and a shorter one inside it
        ctx = plain[0]
        ce, cs = api.Cloud(ctx, _xyzi(world["edge"])), api.Cloud(ctx, _xyzi(world["surf"]))
        p2, f2, s2, b2 = h.init_search_cloud(ce, cs, cands, raw=True)
        assert p2.tobytes() == poses.tobytes() and bytes(f2) == bytes(fit) and s2 == stats and b2 == best
        p3, f3, s3, b3 = h.init_search(world["edge"], world["surf"], cands, raw=True)
        assert p3.tobytes() == poses.tobytes() and bytes(f3) == bytes(fit) and s3 == stats and b3 == best
        assert bytes(h.fitness_cloud(ce, cs, poses, MAX_RANGE, raw=True)) == bytes(fit)
        assert bytes(h.fitness(world["edge"], world["surf"], poses, MAX_RANGE, raw=True)) == bytes(fit)
        # the winner is the rule of the header applied to the reported joint scores
        assert best == ref.winner([_as_dict(x) for x in f[:, 0]])
        # the handle is an aligner still: the single-scan call after the shared-source form is what it was
        one, st1, _ = h.scan_match(world["edge"], world["surf"], cands[0])
        w1, ws1 = h.align_batch([world["edge"]], [world["surf"]], cands[:1])
        assert st1["status"] == 0 and pose_delta(one, w1[0])[0] <= POSE_TOL_M
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ 2. class parity; alone, among 7, among 260
def test_class_entries_are_icp_fitness_and_a_pose_scores_alike_everywhere(loam, world, plain, search7):
    poses7 = search7[0]
    p = poses7[3]
    alone = _fit(loam.fitness(world["edge"], world["surf"], p, MAX_RANGE, raw=True), 1)
    among7 = _fit(loam.fitness(world["edge"], world["surf"], poses7, MAX_RANGE, raw=True), 7)
    many = np.array(world["cands260"])
    many[200] = p  # in the second chunk
    among260 = _fit(loam.fitness(world["edge"], world["surf"], many, MAX_RANGE, raw=True), 260)
    assert alone[0].tobytes() == among7[3].tobytes() == among260[200].tobytes() == _fit(search7[1], 7)[3].tobytes()
    want_surf, want_edge = _class_bits(plain, world, poses7)
    assert among7[:, 1].tobytes() == want_surf.tobytes() and among7[:, 2].tobytes() == want_edge.tobytes()
    one_surf, one_edge = _class_bits(plain, world, p.reshape(1, 7))
    assert alone[0, 1].tobytes() == one_surf.tobytes() and alone[0, 2].tobytes() == one_edge.tobytes()


# ------------------------------------------------------------------------------------------------ 3. the definition
def test_scores_follow_the_definition_at_the_gpus_own_poses(world, search7):
    poses, fit, _, _ = search7
    f = _fit(fit, 7)
    for i in range(7):
        want = world["score"](poses[i])
        for k, name in enumerate(("joint", "surface", "edge")):
            got = _as_dict(f[i, k])
            rel = abs(got["score"] - want[k]["score"]) / want[k]["score"]
            print("candidate %d %-7s score %.9f inliers %d / %d, relative difference to numpy %.2e" % (i, name, got["score"], got["inliers"], got["finite_points"], rel))
            assert (got["inliers"], got["finite_points"]) == (want[k]["inliers"], want[k]["finite_points"]), (i, name, got, want[k])
            assert rel <= SUM_RTOL, (i, name, got, want[k])
        j, s, e = f[i]
        pooled = (s["score"] * s["inliers"] + e["score"] * e["inliers"]) / (s["inliers"] + e["inliers"])
        assert j["inliers"] == s["inliers"] + e["inliers"] and j["finite_points"] == s["finite_points"] + e["finite_points"] == 3215
        assert abs(j["score"] - pooled) <= 1e-12 * pooled, (i, j["score"], pooled)


# ------------------------------------------------------------------------------------------------ 4. the oracle's loop from every candidate
def test_every_candidate_runs_the_oracles_loop(world, search7):
    poses, _, stats, _ = search7
    runs = world["runs7"]
    print("oracle iterations", [r["iterations"] for r in runs], "gpu", [s["iterations"] for s in stats])
    compared = 0
    for i, (r, s) in enumerate(zip(runs, stats)):
        assert r["status"] == 0 and s["status"] == 0
        dt, dr = pose_delta(poses[i], r["pose"])
        if r["iterations"] < loam_ref.LOAM_MAX_ITERATION:  # left through |dx| < eps before the cap; capped runs get no bar
            assert r["converged"]
            print("candidate %d: dt = %.3e m, dr = %.3e rad" % (i, dt, dr))
            assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (i, dt, dr)
            assert s["iterations"] == r["iterations"] and s["converged"], (i, s, r)
            compared += 1
    assert 2 * compared >= 7, compared


# ------------------------------------------------------------------------------------------------ 5. the winner
def test_best_is_the_winner_rule_at_the_oracles_poses(world, search7):
    joint = [f[0] for f in world["fit7"]]
    order = sorted(range(7), key=lambda i: (joint[i]["score"], i))
    win, second = order[0], order[1]
    print("oracle joint scores", ["%.9f" % f["score"] for f in joint], "winner", win, "runner-up", second)
    assert joint[second]["score"] >= (1 + 1e-6) * joint[win]["score"]  # the input's condition: 1000 × the sum bar
    assert ref.winner(joint) == win == search7[3]


# ------------------------------------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("off", ["edge", "surf"])
def test_one_class_switched_off(api, world, plain, off):
    edge, surf = (None, world["surf"]) if off == "edge" else (world["edge"], None)
    h = api.Loam(_opts(api, use_edge_points=int(off != "edge"), use_surf_points=int(off != "surf")))
    try:
        h.set_target(None if off == "edge" else world["edge_map"], None if off == "surf" else world["surf_map"])
        poses, fit, stats, best = h.init_search(edge, surf, world["cands7"], raw=True)
        want_poses, want_stats = h.align_batch(None if edge is None else [edge] * 7, None if surf is None else [surf] * 7, world["cands7"])
        assert poses.tobytes() == want_poses.tobytes() and stats == want_stats
        f = _fit(fit, 7)
        on, gone = (1, 2) if off == "edge" else (2, 1)
        assert f[:, 0].tobytes() == f[:, on].tobytes()
        assert (f[:, gone]["inliers"] == 0).all() and (f[:, gone]["finite_points"] == 0).all() and np.isposinf(f[:, gone]["score"]).all()
        want = _class_bits(plain, world, poses)[0 if off == "edge" else 1]
        assert f[:, on].tobytes() == want.tobytes()
        # a scan handed for the class that is off is not read
        assert bytes(h.fitness(world["edge"], world["surf"], poses, MAX_RANGE, raw=True)) == bytes(fit)
        assert best == ref.winner([_as_dict(x) for x in f[:, 0]]) and best >= 0
    finally:
        h.close()


def test_a_candidate_whose_evaluation_fails_keeps_its_pose_is_scored_there_and_loses(loam, world, locref):
    far = locref.apply_update(world["init"], np.array([0, 0, 0, 500.0, 0, 0]))  # 500 m off the map: no surface point within the plane gate
    r = world["oracle"].scan_match(world["edge"], world["surf"], far, eps=EPS)
    assert r["status"] == 3 and r["iterations"] == 1
    cands = np.vstack([world["cands7"][:2], far[None], world["cands7"][2:4]])
    poses, fit, stats, best = loam.init_search(world["edge"], world["surf"], cands, raw=True)
    f = _fit(fit, 5)
    assert stats[2]["status"] == 3 and stats[2]["iterations"] == 1 and not stats[2]["converged"]
    assert poses[2].tobytes() == far.tobytes()
    assert f[2].tobytes() == _fit(loam.fitness(world["edge"], world["surf"], far, MAX_RANGE, raw=True), 1)[0].tobytes()
    want = world["score"](far)[0]
    assert (int(f[2, 0]["inliers"]), int(f[2, 0]["finite_points"])) == (want["inliers"], want["finite_points"])
    assert best in (0, 1, 3, 4) and all(s["status"] == 0 for i, s in enumerate(stats) if i != 2)
    # ... and a set in which EVERY candidate fails (five edge points) has all outputs filled, each scored where it started
    p5, f5, s5, b5 = loam.init_search(world["edge"][:5], world["surf"], world["cands7"], raw=True)
    assert all(s["status"] == 4 and s["iterations"] == 1 for s in s5) and p5.tobytes() == world["cands7"].tobytes()
    assert bytes(f5) == bytes(loam.fitness(world["edge"][:5], world["surf"], world["cands7"], MAX_RANGE, raw=True))
    assert b5 == ref.winner([_as_dict(x) for x in _fit(f5, 7)[:, 0]])


def test_no_winner_fills_every_output(api, loam, world, search7):
    poses, fit, stats, best = loam.init_search(world["edge"], world["surf"], world["cands7"], api.init_search_opts(min_inlier_ratio=1.1), raw=True)
    assert best == -1 and search7[3] >= 0
    assert poses.tobytes() == search7[0].tobytes() and bytes(fit) == bytes(search7[1]) and stats == search7[2]
    assert all(s["iterations"] > 0 for s in stats) and (_fit(fit, 7)[:, 0]["finite_points"] == 3215).all()


def test_errors_return_the_documented_status(api, world):
    import ctypes
    L = api.lib()
    invalid, no_target = -1, -3
    e, s = np.ascontiguousarray(world["edge"][:64, :3], np.float32), np.ascontiguousarray(world["surf"][:64, :3], np.float32)
    cands = np.ascontiguousarray(world["cands7"])
    out, st, best = np.full((7, 7), 3.0), (api.AlignStats * 7)(), ctypes.c_int(-5)
    fit = (api.Fitness * 21)()
    h = api.Loam(_opts(api))
    try:
        def search(m=7, ne=64, ns=64, sopts=None, pe=e.ctypes.data, ps=s.ctypes.data):
            return L.locgpu_loam_init_search(h._h, pe, ne, ps, ns, 12, cands.ctypes.data, m, ctypes.byref(sopts) if sopts is not None else None, out.ctypes.data, fit, st,
                                             ctypes.byref(best))

        def score(n=7, ne=64, ns=64, max_range=1.0):
            return L.locgpu_loam_fitness(h._h, e.ctypes.data, ne, s.ctypes.data, ns, 12, cands.ctypes.data, n, max_range, fit)

        assert search() == no_target and score() == no_target
        h.set_target(world["edge_map"][:2000], world["surf_map"][:20000])
        assert search(m=0) == invalid and search(m=-2) == invalid and score(n=0) == invalid
        assert search(ne=0, ns=0) == invalid and score(ne=0, ns=0) == invalid
        assert search(pe=None) == invalid  # an enabled class with points and no pointer is refused, not read
        assert score(max_range=float("nan")) == invalid
        for bad in (api.init_search_opts(max_range=float("nan")), api.init_search_opts(min_inlier_ratio=-0.1), api.init_search_opts(min_inlier_ratio=float("nan"))):
            assert search(sopts=bad) == invalid
        assert L.locgpu_loam_init_search(h._h, e.ctypes.data, 64, s.ctypes.data, 64, 12, cands.ctypes.data, 7, None, out.ctypes.data, fit, st, None) == invalid
        assert L.locgpu_loam_init_search_cloud(h._h, None, None, cands.ctypes.data, 7, None, out.ctypes.data, fit, st, ctypes.byref(best)) == invalid
        assert L.locgpu_loam_fitness_cloud(h._h, None, None, cands.ctypes.data, 7, 1.0, fit) == invalid
        assert (out == 3.0).all()  # nothing was written by a refused call
        assert L.locgpu_loam_init_search(None, e.ctypes.data, 64, s.ctypes.data, 64, 12, cands.ctypes.data, 7, None, out.ctypes.data, fit, st, ctypes.byref(best)) == invalid
        # the handle is still good, and an empty scan of ONE enabled class is a score of the other
        assert search(ne=0) == 0 and score(ne=0) == 0
        f = _fit(fit, 7)
        assert (f[:, 2]["finite_points"] == 0).all() and (f[:, 0]["finite_points"] == 64).all()
        with pytest.raises(api.LocGpuError) as err:
            h.fitness_resident(cands[0])  # the storage batches hold the shared-source form
        assert err.value.code == invalid
    finally:
        h.close()


def test_a_handle_on_two_plain_contexts_gives_the_owning_handles_bits(api, world, plain, search7):
    s_ctx, e_ctx = plain
    b = api.Loam.on(s_ctx, e_ctx, _opts(api))
    try:
        poses, fit, stats, best = b.init_search(world["edge"], world["surf"], world["cands7"], raw=True)
        assert poses.tobytes() == search7[0].tobytes() and bytes(fit) == bytes(search7[1]) and stats == search7[2] and best == search7[3]
        one = b.scan_match(world["edge"], world["surf"], world["cands7"][1])
        assert one[1]["status"] == 0
    finally:
        b.close()
    # the contexts outlive the handle, with their targets
    surf_after, edge_after = _class_bits(plain, world, search7[0])
    f = _fit(search7[1], 7)
    assert surf_after.tobytes() == f[:, 1].tobytes() and edge_after.tobytes() == f[:, 2].tobytes()
    # a context without a target is asked at call time
    empty = api.Context(0)
    try:
        b2 = api.Loam.on(s_ctx, empty, _opts(api))
        try:
            with pytest.raises(api.LocGpuError) as err:
                b2.init_search(world["edge"], world["surf"], world["cands7"])
            assert err.value.code == -3
            with pytest.raises(api.LocGpuError) as err:
                b2.fitness(world["edge"], world["surf"], world["cands7"])
            assert err.value.code == -3
            empty.icp_set_target(world["edge_map"])
            assert bytes(b2.fitness(world["edge"], world["surf"], search7[0], MAX_RANGE, raw=True)) == bytes(search7[1])
        finally:
            b2.close()
    finally:
        empty.close()


# ------------------------------------------------------------------------------------------------ 7. façade
def test_cpp_facade_fitness_and_initial_pose_search(world, tmp_path):
    """LoamRegistration::EnableFitnessScore / GetFitnessScore / InitialPoseSearch (tests/cpp/facade_loam_search.cpp): 0.0f without the
    opt-in, ScanMatch byte-identical with and without it, the score that of locgpu_loam_fitness at the result pose, the search what
    locgpu_loam_init_search returns — the driver compares those bit for bit; the values themselves are checked here."""
    exe = os.path.join(os.path.dirname(__file__), "cpp", "facade_loam_search")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    for name in ("edge_map", "surf_map", "edge", "surf"):
        np.ascontiguousarray(world[name][:, :3], dtype=np.float32).tofile(tmp_path / (name + ".bin"))
    np.asarray(world["init"], dtype=np.float64).tofile(tmp_path / "pose.bin")
    np.ascontiguousarray(world["cands7"], dtype=np.float64).tofile(tmp_path / "cands.bin")
    r = subprocess.run([exe] + [str(tmp_path / (n + ".bin")) for n in ("edge_map", "surf_map", "edge", "surf", "pose", "cands", "out")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    out = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    pose, facade_score, abi_score, inliers, finite = out[:7], out[7], out[8], int(out[9]), int(out[10])
    best_pose, best_score, best = out[11:18], out[18], int(out[19])
    want = world["score"](pose)[0]
    assert (inliers, finite) == (want["inliers"], want["finite_points"])
    assert abs(abi_score - want["score"]) <= SUM_RTOL * want["score"]
    assert np.float32(facade_score) == np.float32(abi_score) and facade_score > 0
    assert 0 <= best < 7
    bw = world["score"](best_pose)[0]
    assert abs(best_score - bw["score"]) <= 1e-6 * bw["score"]  # a float32 in the façade's interface
