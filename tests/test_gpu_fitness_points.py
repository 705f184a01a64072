"""The fitness score kernels — icp_fitness_accum_kernel, icp_fitness_sum_kernel, loam_fitness_sum_kernel (csrc/fitness.hip),
ndt_fitness_accum_kernel<NdtOneTarget | NdtVoxelSet> (csrc/ndt_fitness.hip) — and the host arithmetic behind them (gn_driver.hip,
loam_align.hip) PER POINT, at the gates and by the row shapes of the fixed-order sum. Inputs and restatements: tests/fitness_cases.py;
tests/test_fitness_cases_ref.py shows on the CPU that the inputs are what they claim.

The vehicle: a batch of n one-point scans scored with icp_fitness_batch / ndt_fitness_batch is a per-point dump of the accumulate
kernel — for a one-point scan `score` is that point's d² (or χ² residual) when inliers == 1 and +inf otherwise; the division is by 1.0.

  1. ICP per point    float64(d²) of the header's definition by brute force over all map points in float32: the same 8 bytes, inliers
                      == (d² <= float32(max_range²)) with no exclusion near the gate, finite_points == isfinite; max_range 0.3, 1.0, inf.
  2. the gate         exact_world has points with d² == 1.0 and 1.0 + 2^-8 exactly (kept / refused at max_range 1.0); a 16-point world
                      puts fl32(dx·dx) on float32(0.3·0.3) and one float above it.
  3. row shapes       1 … 131 073 points (1 … 129 rows of fixed_order_row_sum) in exact_world, where Σ is an integer sum: alone, in a
                      ragged batch, from a shared source — the same bytes, and those of Σ / inliers formed once from integers. The
                      joint LOAM score likewise. The NDT score has no exact world: bit-identity between the forms, and Σ / inliers
                      against math.fsum of the restatement's per-point minima within u·Σ|x| + u·|score| (the first-order bound of any
                      summation order of the inliers' terms, n·u·Σ|x| / n, and the division).
  4. NDT per point    against the 60-digit restatement fed the GPU's own dumped table, in err / (u·S), S = |e|ᵀ|info||e| +
                      2·|info·e|ᵀ(|R||p| + |t|). Unit 2.5 (the numpy restatement's own worst figure, 2.45, measured on the CPU), bar
                      8 units = 20. The voxel-set kernel gives the single-target kernel's bytes.
  5. the winner       candidates [c1, c0, c0, c1, c0] and the reverse: `best` is the lowest index among the copies of the better pose.

Observed on the MI355X (the whole file: 41 tests, 3 s), worst figure against the bar:

    ICP per point                     bit-equal on 2 464 points x 3 poses x 3 gates (7 points not finite; the two 1e30 rows are finite
                                      points whose d² overflows float32: refused at 0.3 and 1.0, an inlier of score +inf at max_range inf)
    the gate at 1.0                   159 points with d² == 1.0 kept, 336 with d² == 1.0 + 2^-8 refused; whole scans bit-equal
    the gate at 0.3                   fl32(0.300000012²) == float32(0.09) kept on 16 of 16, fl32(0.300000042²) refused on 16 of 16
    ICP rows, ragged, LOAM joint      bit-equal with the integer reference in every form, 1 … 131 073 points
    NDT rows                          the three forms bit-equal; |score − fsum / inliers| at most 0.092 of the bound (3.6e-15 absolute)
    NDT per point                     err / (u·S) 2.22 / 20 with seven voxels probed, 2.22 / 20 with the centre voxel alone; inliers equal
                                      on all 352 points (120 whose smallest residual is not the centre's, 80 rescued by a neighbour, 32 / 112
                                      without an accepted voxel)
    the NDT threshold                 a residual equal to res_outlier_th kept on 8 of 8 voxels, refused with the threshold one double lower
    voxel set                         bit-equal with the single-target kernel, 2 000 points x 3 dealings x 2 nearby types
    the winner                        ICP and NDT: the lowest index among the tied copies, both orders

Mutations tried in scratch builds, one rebuild and one run each, with the existing score tests (test_gpu_fitness.py,
test_gpu_ndt_fitness.py, test_gpu_init_search.py, test_gpu_ndt_init_search.py, test_gpu_loam_init_search.py; their façade tests left out,
and test_fitness_full_size run for the row mutant only) beside this file. What failed here / what failed there:
  `d2 <= gate2` -> `<`                  the per-point ICP tests, both gate tests, every row shape from 255 points, the ragged batch, the
                                        LOAM joint score (21 tests) / nothing
  `res > res_th` -> `>=`                test_ndt_gate_keeps_a_residual_equal_to_the_threshold / nothing
  (dx² + dy²) + dz²                     the three per-point ICP tests / test_fitness_matches_definition and four more, each by a hair:
                                        float32 roundings are 6e-8 a point, the worst sum was 1.003e-9 off against the bar of 1e-9
  the query left in FP64                the three per-point ICP tests / the same existing tests, at 1.0e-9 … 1.3e-9
  the first accepted residual kept      test_ndt_score_per_point_against_60_digits[NEARBY6] / test_ndt_fitness_matches_definition[NEARBY6] and
                                        two more
  `break` after the first row           ICP and NDT rows at 65 537 and 131 073 points, both ragged batches, four LOAM cases (10 tests) /
                                        test_fitness_full_size alone (the 10 M-point map)
  the joint Σ formed edge-first         nothing / nothing: with two classes the joint sum is ONE addition of two doubles, which commutes
                                        bit for bit; the mutant is equivalent and no test can tell it from the code"""
import math

import numpy as np
import pytest

import fitness_cases as cases
import ndt_score_ref

pytestmark = pytest.mark.gpu

FIT = np.dtype([("score", "f8"), ("inliers", "i8"), ("finite_points", "i8")])
CENTER, NEARBY6 = 0, 1
RANGES = (0.3, 1.0, float("inf"))
IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])


def _fit(raw):
    """A ctypes array of locgpu_fitness as a structured array."""
    return np.frombuffer(bytes(raw), dtype=FIT)


def _want(f):
    return np.array([(f["score"], f["inliers"], f["finite_points"])], dtype=FIT)[0]


def _per_point(ctx, scan, poses, call):
    """call(batch, poses) on the batch of len(scan) one-point scans → structured [n]."""
    b = ctx.batch([scan[i:i + 1] for i in range(len(scan))])
    try:
        poses = np.asarray(poses, dtype=np.float64)
        return _fit(call(b, np.stack([poses] * len(scan)) if poses.ndim == 1 else poses))
    finally:
        b.close()


def _show_rows(tag, got, want, rows):
    for i in rows[:8]:
        print("    DIFFERS: %s %d: got %r (score bytes %s), want %r (%s)" % (tag, i, got[i], got[i:i + 1]["score"].tobytes().hex(), want[i], want[i:i + 1]["score"].tobytes().hex()))


# ---------------------------------------------------------------------------------------------- 1. the ICP score per point
@pytest.fixture(scope="module")
def icp_inputs(small_world):
    return cases.icp_point_inputs(small_world)


@pytest.mark.parametrize("pose_name", ["true_pose", "init_pose", "off_0p7m"])
def test_icp_score_per_point_bit_for_bit(gpu_ctx, locref, icp_inputs, pose_name):
    inp, pose = icp_inputs, icp_inputs["poses"][pose_name]
    fin, d2 = cases.icp_point_ref(locref, inp, pose)
    gpu_ctx.icp_set_target(inp["map"])
    for rng in RANGES:
        got = _per_point(gpu_ctx, inp["scan"], pose, lambda b, p: gpu_ctx.icp_fitness_batch(b, p, rng, raw=True))
        with np.errstate(invalid="ignore"):
            inl = fin & (d2 <= cases.gate_of(rng))
        want = np.zeros(len(d2), dtype=FIT)
        want["finite_points"], want["inliers"] = fin, inl
        want["score"] = np.where(inl, d2.astype(np.float64), np.inf)
        bad = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(want))])
        _show_rows("point", got, want, bad)
        print("%s, max_range %s: %s, %d points (%d inliers, %d refused, %d not finite)"
              % (pose_name, rng, "bit-equal" if not len(bad) else "%d DIFFER" % len(bad), len(want), inl.sum(), (fin & ~inl).sum(), (~fin).sum()))
        assert not len(bad), bad[:8]


# ---------------------------------------------------------------------------------------------- 2. the gate
@pytest.fixture(scope="module")
def world():
    """exact_world with the integer d² of every scan point under every pose, for the map and for the edge map."""
    w = cases.exact_world()
    w["d2"] = [cases.exact_d2(w["grid"], cases.exact_apply(p, w["src_int"])) for p in w["poses"]]
    w["d2_edge"] = [cases.exact_d2(w["edge_grid"], cases.exact_apply(p, w["src_int"])) for p in w["poses"]]
    return w


def test_gate_keeps_a_squared_distance_equal_to_max_range_squared(gpu_ctx, world):
    """`d2 <= gate2`: d² == 1.0 exactly is an inlier at max_range 1.0, d² == 1.0 + 2^-8 is not; per point, then as whole scans."""
    gpu_ctx.icp_set_target(world["map"])
    pose, d2 = world["poses"][1][0], world["d2"][1]
    at, above = np.flatnonzero(d2 == cases.Q2), np.flatnonzero(d2 == cases.Q2 + 1)
    assert len(at) >= 100 and len(above) >= 100
    call = lambda b, p: gpu_ctx.icp_fitness_batch(b, p, 1.0, raw=True)  # noqa: E731
    got_at, got_above = _per_point(gpu_ctx, world["src"][at], pose, call), _per_point(gpu_ctx, world["src"][above], pose, call)
    print("d2 == 1.0: %d points, %d kept; d2 == 1.0 + 2^-8: %d points, %d kept" % (len(at), got_at["inliers"].sum(), len(above), got_above["inliers"].sum()))
    assert (got_at["inliers"] == 1).all() and (got_at["score"] == 1.0).all() and (got_at["finite_points"] == 1).all()
    assert (got_above["inliers"] == 0).all() and np.isposinf(got_above["score"]).all() and (got_above["finite_points"] == 1).all()
    for tag, rows in (("at the gate", at), ("one step above", above), ("both", np.r_[at, above]), ("the first 4096 points", np.arange(4096))):
        f, _ = cases.exact_fitness(d2[rows], 1.0)
        got = _fit(gpu_ctx.icp_fitness(world["src"][rows], pose.reshape(1, 7), 1.0, raw=True))[0]
        print("%s: got %r, integer reference %r" % (tag, got, f))
        assert got.tobytes() == _want(f).tobytes()
    print("bit-equal, %d points" % (len(at) + len(above)))


def test_gate_that_is_no_dyadic_number(gpu_ctx):
    """max_range 0.3: the gate is float32(0.3·0.3) formed in double and cast once. fl32(dx·dx) == gate is kept, the next float's is not."""
    dx_at, dx_above = cases.gate_neighbours(0.3)
    gate = cases.gate_of(0.3)
    m, at, above = cases.gate_world(dx_at, dx_above)
    gpu_ctx.icp_set_target(m)
    call = lambda b, p: gpu_ctx.icp_fitness_batch(b, p, 0.3, raw=True)  # noqa: E731
    got = _per_point(gpu_ctx, np.concatenate([at, above]), IDENT, call)
    print("gate %.9g: dx %.9g kept on %d of 16, dx %.9g kept on %d of 16" % (gate, dx_at, got["inliers"][:16].sum(), dx_above, got["inliers"][16:].sum()))
    assert got["inliers"].tolist() == [1] * 16 + [0] * 16 and (got["finite_points"] == 1).all()
    assert (got["score"][:16] == float(gate)).all() and np.isposinf(got["score"][16:]).all()
    for s, n in ((at, 16), (above, 0), (np.concatenate([at, above]), 16)):
        f = gpu_ctx.icp_fitness(s, IDENT, 0.3)
        assert f == dict(score=float(gate) if n else float("inf"), inliers=n, finite_points=len(s)), f
    print("bit-equal, 32 points")


# ---------------------------------------------------------------------------------------------- 3. row shapes of the fixed-order sum
@pytest.mark.parametrize("n", cases.ROW_LENGTHS)
def test_icp_row_shapes_sum_to_the_integer_reference(gpu_ctx, world, n):
    """A scan of n points alone and from a shared source of 3 entries (one pose each): the bytes of Σ / inliers from exact integers."""
    gpu_ctx.icp_set_target(world["map"])
    s = world["src"][:n]
    poses = np.stack([p[0] for p in world["poses"]])
    for rng in (1.0, 0.3, float("inf")):
        want = [_want(cases.exact_fitness(world["d2"][k][:n], rng)[0]) for k in range(3)]
        alone = [_fit(gpu_ctx.icp_fitness(s, poses[k].reshape(1, 7), rng, raw=True))[0] for k in range(3)]
        among = _fit(gpu_ctx.icp_fitness(s, poses, rng, raw=True))
        sh = gpu_ctx.batch_shared(s, 3)
        try:
            shared = _fit(gpu_ctx.icp_fitness_batch(sh, poses, rng, raw=True))
        finally:
            sh.close()
        for k in range(3):
            same = alone[k].tobytes() == among[k].tobytes() == shared[k].tobytes() == want[k].tobytes()
            if not same:
                print("    DIFFERS: n %d pose %d max_range %s: alone %r, among three poses %r, shared source %r, integer reference %r" % (n, k, rng, alone[k], among[k], shared[k], want[k]))
            assert same, (n, k, rng)
    print("n = %d (%d rows): bit-equal, %d points x 3 poses x 3 gates x 3 forms" % (n, (n + 1023) // 1024, n))


def test_icp_ragged_batch_sums_to_the_integer_reference(gpu_ctx, world):
    """131 073, 65 537, 1 025, 1 and 0 points in one batch: the short scans own rows that exist only as zeros."""
    gpu_ctx.icp_set_target(world["map"])
    starts = (0, 1000, 5, 7, 0)
    scans = [world["src"][a:a + n] for a, n in zip(starts, cases.RAGGED)]
    which = [1, 2, 0, 1, 2]
    poses = np.stack([world["poses"][k][0] for k in which])
    for order in (range(5), reversed(range(5))):
        order = list(order)
        b = gpu_ctx.batch([scans[i] for i in order])
        try:
            for rng in (1.0, float("inf")):
                got = _fit(gpu_ctx.icp_fitness_batch(b, poses[order], rng, raw=True))
                for j, i in enumerate(order):
                    a, n = starts[i], cases.RAGGED[i]
                    want = _want(cases.exact_fitness(world["d2"][which[i]][a:a + n], rng)[0])
                    alone = _fit(gpu_ctx.icp_fitness(scans[i], poses[i].reshape(1, 7), rng, raw=True))[0] if n else want
                    if not got[j].tobytes() == alone.tobytes() == want.tobytes():
                        print("    DIFFERS: ragged, max_range %s, %d points: batch %r, alone %r, integer reference %r" % (rng, n, got[j], alone, want))
                    assert got[j].tobytes() == alone.tobytes() == want.tobytes(), (i, rng)
        finally:
            b.close()
    print("bit-equal, %d points" % sum(cases.RAGGED))


def _loam_opts(api, **kw):
    return api.loam_opts(surf=api.icp_opts(method=api.P2PLANE), edge=api.icp_opts(method=api.P2LINE), **kw)


@pytest.mark.parametrize("case", ["edge_1_row_surf_65_rows", "edge_65_rows_surf_1_row", "empty_edge", "edge_off", "surf_off"])
def test_loam_joint_score_is_the_integer_sum_of_both_classes(api, gpu_ctx, world, case):
    """joint.score == (Σ_surf + Σ_edge) / (inl_surf + inl_edge) from integers; the class entries are icp_fitness of a plain context."""
    n_edge, n_surf = {"edge_1_row_surf_65_rows": (1000, 65537), "edge_65_rows_surf_1_row": (65537, 1000), "empty_edge": (0, 1025),
                      "edge_off": (1000, 65537), "surf_off": (65537, 1000)}[case]
    edge, surf = world["src"][2000:2000 + n_edge], world["src"][500:500 + n_surf]
    use_edge, use_surf = case != "edge_off", case != "surf_off"
    poses = np.stack([p[0] for p in world["poses"]])
    h = api.Loam(_loam_opts(api, use_edge_points=int(use_edge), use_surf_points=int(use_surf)))
    plain_edge = api.Context(0)
    try:
        h.set_target(world["edge_map"] if use_edge else None, world["map"] if use_surf else None)
        gpu_ctx.icp_set_target(world["map"])
        plain_edge.icp_set_target(world["edge_map"])
        for rng in (1.0, float("inf")):
            got = _fit(h.fitness(edge, surf, poses, rng, raw=True)).reshape(3, 3)
            for k in range(3):
                fs, ps = cases.exact_fitness(world["d2"][k][500:500 + n_surf], rng) if use_surf else (dict(score=float("inf"), inliers=0, finite_points=0), (0, 0))
                fe, pe = cases.exact_fitness(world["d2_edge"][k][2000:2000 + n_edge], rng) if use_edge else (dict(score=float("inf"), inliers=0, finite_points=0), (0, 0))
                fj = cases.joint_fitness([ps + (fs["finite_points"],), pe + (fe["finite_points"],)])
                want = [_want(fj), _want(fs), _want(fe)]
                if any(got[k, c].tobytes() != want[c].tobytes() for c in range(3)):
                    print("    DIFFERS: %s, pose %d, max_range %s: joint %r surface %r edge %r; integer reference %r %r %r" % (case, k, rng, got[k, 0], got[k, 1], got[k, 2], fj, fs, fe))
                for c in range(3):
                    assert got[k, c].tobytes() == want[c].tobytes(), (case, k, rng, c)
                if use_surf:
                    assert got[k, 1].tobytes() == _fit(gpu_ctx.icp_fitness(surf, poses[k].reshape(1, 7), rng, raw=True))[0].tobytes()
                if use_edge and n_edge:
                    assert got[k, 2].tobytes() == _fit(plain_edge.icp_fitness(edge, poses[k].reshape(1, 7), rng, raw=True))[0].tobytes()
    finally:
        h.close()
        plain_edge.close()
    print("bit-equal, %d + %d points x 3 poses x 2 gates" % (n_surf if use_surf else 0, n_edge if use_edge else 0))


@pytest.fixture(scope="module")
def ndt_rows(gpu_ctx, api, locref, small_world):
    """The NDT row-shape world: the small world's first 20 000 map points as the target (NEARBY6), the GPU's own dump of it, scan2k
    rolled to start at an inlier of true_pose, and the restatement's per-point minima under true_pose and init_pose."""
    m = np.ascontiguousarray(small_world["map"][:20000])
    gpu_ctx.ndt_set_target(m, api.ndt_opts(nearby_type=NEARBY6))
    table = ndt_score_ref.Table(*gpu_ctx.ndt_dump())
    s = np.ascontiguousarray(np.asarray(small_world["scan2k"], dtype=np.float32)[:, :3])
    poses = np.stack([small_world["true_pose"], small_world["init_pose"]])
    first = int(cases.classify(ndt_score_ref.residuals(locref, table, s, poses[0], cases.VOXEL, 7))[1].argmax())
    s = np.roll(s, -first, axis=0)
    best = []
    for pose in poses:
        res = ndt_score_ref.residuals(locref, table, s, pose, cases.VOXEL, 7)
        assert ndt_score_ref.gate_margin(res, cases.RES_TH) > cases.GATE_REL * cases.RES_TH  # conditions on the input, decided on the CPU
        frac = locref.transform_points(pose, s.astype(np.float64)) / cases.VOXEL
        assert np.abs(frac - np.rint(frac)).min() > cases.KEY_MARGIN
        best.append(cases.classify(res)[0])
    assert np.isfinite(best[0][0])
    return dict(map=m, scan=s, poses=poses, best=best)


def _ndt_target(gpu_ctx, api, ndt_rows):
    gpu_ctx.ndt_set_target(ndt_rows["map"], api.ndt_opts(nearby_type=NEARBY6))


def _ndt_sum_check(tag, got, best, n):
    """Σ / inliers of the first n points of the tiled scan against math.fsum of the restatement's minima."""
    x = np.tile(best, n // len(best) + 1)[:n]  # the scan is tiled to length, and so are its minima
    x = x[np.isfinite(x)]
    assert got["inliers"] == len(x) and got["finite_points"] == n, (tag, got, len(x))
    if not len(x):
        assert np.isposinf(got["score"])
        return 0.0
    ref = math.fsum(x) / len(x)
    tol = cases.U * math.fsum(np.abs(x)) + cases.U * abs(ref)
    err = abs(float(got["score"]) - ref)
    print("%s: %d inliers of %d, |score - fsum / inliers| %.3e, bound %.3e (%.3g of it)" % (tag, len(x), n, err, tol, err / tol))
    assert err <= tol, (tag, err, tol)
    return err / tol


@pytest.mark.parametrize("n", cases.ROW_LENGTHS)
def test_ndt_row_shapes(gpu_ctx, api, ndt_rows, n):
    _ndt_target(gpu_ctx, api, ndt_rows)
    s = cases.tiled(ndt_rows["scan"], n)
    poses = ndt_rows["poses"][[0, 1, 0]]
    alone = [_fit(gpu_ctx.ndt_fitness(s, poses[k].reshape(1, 7), raw=True))[0] for k in range(3)]
    sh, cp = gpu_ctx.batch_shared(s, 3), gpu_ctx.batch([s, s[:max(n // 2, 1)], s])
    try:
        shared = _fit(gpu_ctx.ndt_fitness_batch(sh, poses, raw=True))
        copies = _fit(gpu_ctx.ndt_fitness_batch(cp, poses, raw=True))
    finally:
        sh.close()
        cp.close()
    for k in range(3):
        assert alone[k].tobytes() == shared[k].tobytes(), (n, k, alone[k], shared[k])
        if k != 1:
            assert alone[k].tobytes() == copies[k].tobytes(), (n, k, alone[k], copies[k])
        _ndt_sum_check("n = %d (%d rows), pose %d" % (n, (n + 1023) // 1024, k), alone[k], ndt_rows["best"][(0, 1, 0)[k]], n)


def test_ndt_ragged_batch(gpu_ctx, api, ndt_rows):
    _ndt_target(gpu_ctx, api, ndt_rows)
    scans = [cases.tiled(ndt_rows["scan"], n) for n in cases.RAGGED]
    which = [0, 1, 0, 0, 1]
    poses = ndt_rows["poses"][which]
    b = gpu_ctx.batch(scans)
    try:
        got = _fit(gpu_ctx.ndt_fitness_batch(b, poses, raw=True))
    finally:
        b.close()
    for i, n in enumerate(cases.RAGGED):
        _ndt_sum_check("ragged, %d points" % n, got[i], ndt_rows["best"][which[i]], n)
        if n:
            assert got[i].tobytes() == _fit(gpu_ctx.ndt_fitness(scans[i], poses[i].reshape(1, 7), raw=True))[0].tobytes(), n
        else:
            assert got[i].tobytes() == _want(dict(score=float("inf"), inliers=0, finite_points=0)).tobytes()


# ---------------------------------------------------------------------------------------------- 4. the NDT score per point
@pytest.mark.parametrize("nearby", [NEARBY6, CENTER])
def test_ndt_score_per_point_against_60_digits(gpu_ctx, api, locref, small_world, nearby):
    n_nearby = 7 if nearby == NEARBY6 else 1
    gpu_ctx.ndt_set_target(small_world["map"], api.ndt_opts(nearby_type=nearby))
    table = ndt_score_ref.Table(*gpu_ctx.ndt_dump())  # data here; the records are tested in test_gpu_ndt_voxels.py
    bar = cases.BAR_FACTOR * cases.UNIT
    worst, counts = 0.0, np.zeros(3, dtype=int)
    for name, pose, pts in cases.ndt_point_inputs(locref, table, small_world):
        r = cases.ndt_point_ref(table, pts, pose, n_nearby)
        # conditions on the input, from the restatement alone: nothing is excluded
        assert r["key_margin"].min() > cases.KEY_MARGIN and r["gate_margin"].min() > cases.GATE_REL
        _, which, nc, rs, no = cases.classify(r["res"])
        counts += [nc.sum(), rs.sum(), no.sum()]
        got = _per_point(gpu_ctx, pts, pose, lambda b, p: gpu_ctx.ndt_fitness_batch(b, p, raw=True))
        assert (got["finite_points"] == 1).all()
        wrong = np.flatnonzero(got["inliers"] != r["inlier"])
        assert not len(wrong), (name, wrong[:8], got[wrong[:8]], r["best"][wrong[:8]])
        assert np.isposinf(got["score"][~r["inlier"]]).all()
        un = np.zeros(len(pts))
        for i in np.flatnonzero(r["inlier"]):
            un[i] = cases.err_in_units(got["score"][i], r["best_mp"][i], r["S"][i, r["which"][i]])
        for i in np.flatnonzero(un > bar)[:8]:
            print("    ABOVE THE BAR: point %d = %s, %.3g units, got %.17g, want %.17g (voxel %d of the probe order), all residuals %s"
                  % (i, pts[i].tolist(), un[i], got["score"][i], r["best"][i], r["which"][i], r["res"][i].tolist()))
        print("%s, %d voxels probed: %d points (%d inliers; smallest not the centre's %d, centre refused or absent and a neighbour accepted %d, none accepted %d): "
              "worst err / (u S) %.3g (bar %.3g = 8 x %.3g)" % (name, n_nearby, len(pts), r["inlier"].sum(), nc.sum(), rs.sum(), no.sum(), un.max(), bar, cases.UNIT))
        assert un.max() <= bar
        worst = max(worst, un.max())
    if nearby == NEARBY6:
        assert counts[0] >= 50 and counts[1] >= 20 and counts[2] >= 20, counts
    else:
        assert counts[2] >= 20, counts
    print("worst err / (u S) %.3g, bar %.3g" % (worst, bar))


def test_ndt_gate_keeps_a_residual_equal_to_the_threshold(gpu_ctx, api, small_world):
    """`res > res_th` refuses: a residual EQUAL to res_outlier_th is kept, and refused under the next double below as the threshold. The
    residual is exact by design (fitness_cases.ndt_gate_cases): e has one non-zero component. The threshold is an option of the ingest,
    so the record is read back after the ingest that set it, and the threshold is the value of THAT record."""
    m = np.ascontiguousarray(small_world["map"][:20000])
    gpu_ctx.ndt_set_target(m, api.ndt_opts(nearby_type=CENTER))
    first = gpu_ctx.ndt_dump()
    gate = cases.ndt_gate_cases(ndt_score_ref.Table(*first))
    assert len(gate) == 8
    origin = np.zeros((1, 3), np.float32)
    kept = refused = 0
    for t, th, key in gate:
        for _ in range(3):  # a condition on the input: the threshold set is the residual of the record as ingested under it
            gpu_ctx.ndt_set_target(m, api.ndt_opts(nearby_type=CENTER, res_outlier_th=th))
            dump = gpu_ctx.ndt_dump()
            table = ndt_score_ref.Table(*dump)
            t, again = cases.ndt_gate_case(table, int(np.searchsorted(table.packed, key)))
            if again == th:
                break
            print("    the re-ingested records differ from the first ingest's in %s rows (keys, mu, info); threshold %.17g -> %.17g"
                  % ([int((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1).sum()) if a.shape == b.shape else -1 for a, b in zip(first, dump)], th, again))
            th = again
        assert again == th
        pose = np.concatenate([[0, 0, 0, 1.0], t])
        at = _fit(gpu_ctx.ndt_fitness(origin, pose.reshape(1, 7), raw=True))[0]
        gpu_ctx.ndt_set_target(m, api.ndt_opts(nearby_type=CENTER, res_outlier_th=float(np.nextafter(th, 0.0))))
        below = _fit(gpu_ctx.ndt_fitness(origin, pose.reshape(1, 7), raw=True))[0]
        print("voxel key %d, threshold %.17g: at the threshold %r, threshold one double lower %r" % (key, th, at, below))
        kept, refused = kept + int(at["inliers"]), refused + int(below["inliers"] == 0)
        assert at.tobytes() == _want(dict(score=th, inliers=1, finite_points=1)).tobytes()
        assert below.tobytes() == _want(dict(score=float("inf"), inliers=0, finite_points=1)).tobytes()
    print("bit-equal, %d points kept at the threshold, %d refused with the threshold one double lower" % (kept, refused))


@pytest.mark.parametrize("nearby", [NEARBY6, CENTER])
def test_voxel_set_kernel_gives_the_single_target_bytes(gpu_ctx, api, small_world, nearby):
    """ndt_fitness_pairs on a two-target set: the one-point batch under target 0, under target 1 and dealt over both."""
    opts = api.ndt_opts(nearby_type=nearby)
    targets = [np.ascontiguousarray(small_world["map"][:100000]), np.ascontiguousarray(small_world["map"][100000:])]
    s = np.ascontiguousarray(np.asarray(small_world["scan2k"], dtype=np.float32)[:, :3])
    poses = np.stack([small_world["true_pose"] if i % 3 else small_world["init_pose"] for i in range(len(s))])
    single = []
    for t in targets:
        gpu_ctx.ndt_set_target(t, opts)
        single.append(_per_point(gpu_ctx, s, poses, lambda b, p: gpu_ctx.ndt_fitness_batch(b, p, raw=True)))
    assert single[0].tobytes() != single[1].tobytes() and single[0]["inliers"].sum() > 100 and single[1]["inliers"].sum() > 100
    c = api.Context(0)
    try:
        c.ndt_set_target_set(targets, opts)
        dealt = np.arange(len(s)) % 2
        for tag, target_of in (("target 0", np.zeros(len(s), int)), ("target 1", np.ones(len(s), int)), ("dealt over both", dealt)):
            got = _per_point(c, s, poses, lambda b, p: c.ndt_fitness_pairs(b, target_of, p, raw=True))
            want = np.where(target_of == 0, single[0], single[1])
            bad = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(s))])
            _show_rows(tag, got, want, bad)
            print("%s: %s, %d points (%d inliers)" % (tag, "bit-equal" if not len(bad) else "%d DIFFER" % len(bad), len(s), want["inliers"].sum()))
            assert not len(bad)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------- 5. the winner rule meets a tie
def _tie_check(tag, search, c0, c1):
    for order in ([1, 0, 0, 1, 0], [0, 1, 0, 0, 1]):
        cands = np.stack([c1 if k else c0 for k in order])
        poses, fit, stats, best = search(cands)
        f = _fit(fit)[:5]
        a, b = order.index(0), order.index(1)
        for i, k in enumerate(order):  # equal candidates: equal bytes of pose and score
            assert poses[i].tobytes() == poses[a if k == 0 else b].tobytes() and f[i].tobytes() == f[a if k == 0 else b].tobytes()
        ok = [i for i in range(5) if f[i]["inliers"] > 0 and f[i]["inliers"] >= 0.25 * f[i]["finite_points"]]
        assert len(ok) == 5  # every candidate qualifies: the score alone decides
        assert f[a]["score"] != f[b]["score"]  # one pose is the better one
        better = 0 if f[a]["score"] < f[b]["score"] else 1
        want = order.index(better)
        print("%s, candidates %s: scores %s, best %d, want %d (the lowest index among the %d copies of the better pose)"
              % (tag, order, ["%.9g" % v for v in f["score"]], best, want, order.count(better)))
        assert order.count(better) >= 2 or order.count(1 - better) >= 2
        assert best == want == ndt_score_ref.winner([dict(score=float(x["score"]), inliers=int(x["inliers"]), finite_points=int(x["finite_points"])) for x in f], 0.25)


def test_icp_winner_is_the_lowest_index_among_tied_candidates(gpu_ctx, api, world):
    gpu_ctx.icp_set_target(world["map"])
    s = world["src"][:4096]
    c0 = world["poses"][1][0]
    c1 = np.array(c0, copy=True)
    c1[4:] += [0.1875, -0.125, 0.0625]
    sopts = api.init_search_opts(min_inlier_ratio=0.25)
    _tie_check("ICP P2P", lambda cands: gpu_ctx.icp_init_search(s, cands, api.icp_opts(method=api.P2P), sopts, raw=True), c0, c1)


def test_ndt_winner_is_the_lowest_index_among_tied_candidates(gpu_ctx, api, small_world):
    gpu_ctx.ndt_set_target(small_world["map"], api.ndt_opts(nearby_type=NEARBY6))
    s = small_world["scan2k"]
    sopts = api.init_search_opts(min_inlier_ratio=0.25)
    _tie_check("NDT", lambda cands: gpu_ctx.ndt_init_search(s, cands, sopts, raw=True), np.asarray(small_world["true_pose"], dtype=np.float64),
               np.asarray(small_world["init_pose"], dtype=np.float64))
