"""locgpu_ndt_hb / locgpu_ndt_hb_batch — one iteration's H, B, effective_num, ok of ndt_accum_kernel (direct NDT) and inc_accum_kernel
(incremental NDT) behind gn_solve_kernel — against the oracle's locref.Ndt.hb and, per point, against the long-double restatement of
tests/ndt_hb_ref.py.

Bars. Aggregates (sums over a scan): test_gpu_parity._hb_close, H to 1e-9 of max|H|, B to 1e-8 of max(|B|, 1e-6·max|H|). Integers
(effective_num, ok, the number of accepted (point, voxel) pairs) exactly. Per point: 8 units, a unit being the ORACLE's own worst
per-point error against the restatement on the same 512 points (measured by test_ndt_hb_ref.py::test_per_point_unit_of_the_oracle,
recorded in ndt_hb_cases.UNIT), H relative to max|H_point|, B relative to max(|B_point|, sqrt(max|H_point|)):

    direct NDT       unit H 4.9e-16, B 1.9e-14   →  bar H 3.92e-15, B 1.52e-13
    incremental NDT  unit H 9.0e-16, B 1.18e-13  →  bar H 7.20e-15, B 9.44e-13

Both sides are FP64 evaluations of one formula that differ in grouping by a handful of roundings. Observed on the MI355X: per point
direct H 4.1e-16, B 1.8e-14, incremental H 3.8e-16, B 1.18e-13 (about one unit); aggregates at the worst 5.0e-14 of max|H| and 1.4e-14
of B's scale (an iterate of the direct NEARBY6 alignment). Every test prints its worst observed
differences next to its bars."""
import numpy as np
import pytest

import ndt_hb_cases as cases
import ndt_hb_ref as ref
from test_gpu_parity import HB_RTOL, _hb_close

pytestmark = pytest.mark.gpu

ALL = list(cases.CASES)
ONE_EACH = ["direct_nearby6", "inc_th5"]


@pytest.fixture(scope="module")
def oracles(locref, synth, small_world):
    return {name: cases.oracle_target(locref, synth, small_world, name) for name in cases.CASES}


def _target(gpu_ctx, api, locref, synth, small_world, name, extra=None):
    cases.gpu_target(gpu_ctx, api, locref, synth, small_world, name, extra)


def _row(row):
    """A 44-double row of ndt_hb_batch as ndt_hb returns it: (ok, H, B, effective_num)."""
    return bool(row[43]), row[:36].reshape(6, 6), row[36:42], int(row[42])


def _aggregate(tag, got, want, with_ok=True):
    """got / want: (ok, H, B, effective_num). Prints the differences, then holds them to the aggregate bars; returns them."""
    ok_g, Hg, Bg, eff_g = got
    ok_o, Ho, Bo, eff_o = want
    scale = max(np.abs(Ho).max(), 1e-300)
    scale_b = max(np.abs(Bo).max(), np.abs(Ho).max() * 1e-6, 1e-300)
    dh, db = np.abs(Hg - Ho).max() / scale, np.abs(Bg - Bo).max() / scale_b
    print("%s: |dH|/max|H| %.2e (bar %.0e)  |dB|/scale %.2e (bar 1e-08)  effective_num %d / %d  ok %s / %s" % (tag, dh, HB_RTOL, db, eff_g, eff_o, ok_g, ok_o))
    assert np.isfinite(Hg).all() and np.isfinite(Bg).all()
    _hb_close(Hg, Bg, Ho, Bo)
    assert eff_g == eff_o
    if with_ok:
        assert ok_g == ok_o
    return dh, db


# ---------------------------------------------------------------------------------------------- 3.1 every iterate of an alignment
@pytest.mark.parametrize("name", ALL)
def test_every_iterate_of_an_alignment(gpu_ctx, api, locref, synth, small_world, oracles, name):
    """The oracle's trace rows (H, B, effective_num, ok of every iteration, the converged one included) at the oracle's own iterates."""
    ndt, scan = oracles[name], small_world["scan10k"]
    _target(gpu_ctx, api, locref, synth, small_world, name)
    ro = ndt.align(scan, small_world["init_pose"], trace_cap=20)
    assert ro["status"] == 0 and len(ro["trace"]) == ro["iters"] >= 5
    pose = np.array(small_world["init_pose"], dtype=np.float64)
    worst = [0.0, 0.0]
    for it, row in enumerate(ro["trace"]):
        Ho, Bo, dx, eff_o, ok_o = row[:36].reshape(6, 6), row[36:42], row[42:48], int(row[48]), bool(row[49])
        ok_g, Hg, Bg, eff_g = gpu_ctx.ndt_hb(scan, pose)
        dh, db = _aggregate("%s iteration %d" % (name, it), (ok_g, Hg, Bg, eff_g), (ok_o, Ho, Bo, eff_o))
        worst = [max(worst[0], dh), max(worst[1], db)]
        assert np.array_equal(Hg, Hg.T)
        pairs_g, pairs_o = cases.accepted_pairs(name, Hg, eff_g), cases.accepted_pairs(name, Ho, eff_o)
        print("    accepted (point, voxel) pairs %d / %d" % (pairs_g, pairs_o))
        assert pairs_g == pairs_o  # the gate's exact witness
        pose = locref.apply_update(pose, dx)
    np.testing.assert_array_equal(pose, ro["pose"])  # the iterates rebuilt here are the oracle's
    print("%s: worst over %d iterates |dH| %.2e, |dB| %.2e" % (name, ro["iters"], worst[0], worst[1]))


# ---------------------------------------------------------------------------------------------- 3.2 per point
@pytest.mark.parametrize("name", ALL)
def test_per_point_against_the_long_double_restatement(gpu_ctx, api, locref, synth, small_world, oracles, name):
    """A batch of 512 one-point scans is a per-point dump of the accumulate kernel. `ok` is not compared: a one-point H has rank 3, and
    det == 0 there is a rounding accident on either side."""
    method, _, th = cases.CASES[name]
    pts, pose = cases.sample_points(small_world)
    pp = cases.restate(oracles[name], name, pts, pose)
    excluded = ref.near_gate(pp["res"], th, cases.GATE_REL)
    assert excluded.mean() <= cases.MAX_EXCLUDED and (pp["n_acc"] > 0).sum() >= 256  # conditions of the input, from the restatement alone
    _target(gpu_ctx, api, locref, synth, small_world, name)
    b = gpu_ctx.batch([pts[i:i + 1] for i in range(len(pts))])
    try:
        hb = gpu_ctx.ndt_hb_batch(b, np.stack([pose] * len(pts)))
    finally:
        b.close()
    H, B, eff = hb[:, :36].reshape(-1, 6, 6), hb[:, 36:42], hb[:, 42]
    assert np.isfinite(hb).all()
    got = np.array([cases.accepted_pairs(name, H[i], eff[i]) for i in range(len(pts))])
    keep = ~excluded
    print("%s: accepted voxels per point differ on %d of %d compared points (%d excluded near the gate)" % (name, int((got[keep] != pp["n_acc"][keep]).sum()), int(keep.sum()), int(excluded.sum())))
    assert np.array_equal(got[keep], pp["n_acc"][keep])
    if method == 1:
        assert (eff == 1).all()
    eh, eb = ref.point_errors(H, B, pp)
    uh, ub = cases.UNIT[method]
    bar_h, bar_b = cases.BAR_FACTOR * uh, cases.BAR_FACTOR * ub
    print("%s: worst per-point error H %.3e (bar %.2e = 8 x %.2e), B %.3e (bar %.2e = 8 x %.2e)" % (name, eh[keep].max(), bar_h, uh, eb[keep].max(), bar_b, ub))
    assert eh[keep].max() <= bar_h and eb[keep].max() <= bar_b
    assert np.array_equal(H, H.transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------- 3.3 points-per-thread rungs
@pytest.fixture(scope="module")
def scan8193(synth):
    s = synth.make_scan(3, subsample=8193, crop_half=36.0)
    assert len(s) == 8193  # 33 blocks of 256, the last one holding one point
    return s


@pytest.fixture(scope="module")
def rung_refs(locref, small_world, oracles, scan8193):
    """The oracle at the eight poses, once per target."""
    poses = cases.perturbed_poses(locref, small_world["init_pose"], 8)
    assert len({p.tobytes() for p in poses}) == 8
    return poses, {name: [oracles[name].hb(scan8193, p) for p in poses] for name in ONE_EACH}


@pytest.mark.parametrize("name,n_entries", [("direct_nearby6", 32), ("direct_nearby6", 64), ("direct_nearby6", 128), ("direct_nearby6", 256),
                                            ("inc_th5", 32), ("inc_th5", 256)])
def test_points_per_thread_rungs(gpu_ctx, api, locref, synth, small_world, scan8193, rung_refs, name, n_entries):
    """33 blocks per entry x 32, 64, 128, 256 entries = 1 056, 2 112, 4 224, 8 448 blocks: ndt_accum_kernel sums 1, 2, 4, 8 points per
    thread (launch_ndt_accum), and with 8 the grid's last column covers blocks 32-39 of which one exists. The incremental kernel has no
    such loop but reads the shared source the same way."""
    poses, want = rung_refs
    _target(gpu_ctx, api, locref, synth, small_world, name)
    b = gpu_ctx.batch_shared(scan8193, n_entries)
    try:
        hb = gpu_ctx.ndt_hb_batch(b, poses[np.arange(n_entries) % 8])
    finally:
        b.close()
    worst = [0.0, 0.0]
    for e in range(n_entries):
        got, ref_e = _row(hb[e]), want[name][e % 8]
        if e < 8:
            dh, db = _aggregate("%s x%d entry %d" % (name, n_entries, e), got, ref_e)
            worst = [max(worst[0], dh), max(worst[1], db)]
        else:  # every entry is held to the oracle; the later ones print nothing
            _hb_close(got[1], got[2], ref_e[1], ref_e[2])
            assert got[0] == ref_e[0] and got[3] == ref_e[3], e
            assert hb[e].tobytes() == hb[e % 8].tobytes(), e  # the same pose: the same bits, wherever the entry sits in the grid
        assert cases.accepted_pairs(name, got[1], got[3]) == cases.accepted_pairs(name, ref_e[1], ref_e[3]), e
    print("%s x%d: all %d entries equal the oracle at their pose, worst |dH| %.2e (bar %.0e), |dB| %.2e (bar 1e-08); entries 8.. are bit-identical "
          "to the first entry of their pose" % (name, n_entries, n_entries, worst[0], HB_RTOL, worst[1]))


# ---------------------------------------------------------------------------------------------- 3.4 ragged sizes
@pytest.mark.parametrize("name", ONE_EACH)
def test_ragged_batch_around_the_launch_shape(gpu_ctx, api, locref, synth, small_world, oracles, name):
    sizes = [1, 63, 64, 65, 255, 256, 257, 513]
    s2k, pose = small_world["scan2k"], small_world["true_pose"]
    scans, at = [], 0
    for n in sizes:
        scans.append(np.ascontiguousarray(s2k[at:at + n]))
        at += n
    assert at <= len(s2k)
    _target(gpu_ctx, api, locref, synth, small_world, name)
    b = gpu_ctx.batch(scans)
    try:
        hb = gpu_ctx.ndt_hb_batch(b, np.stack([pose] * len(scans)))
    finally:
        b.close()
    min_pts = 10  # min_effective_pts of the default options
    for i, sc in enumerate(scans):
        ok1, H1, B1, eff1 = gpu_ctx.ndt_hb(sc, pose)
        ok, H, B, eff = _row(hb[i])
        assert H.tobytes() == H1.tobytes() and B.tobytes() == B1.tobytes() and eff == eff1 and ok == ok1, sizes[i]
        # below min_effective_pts H may be singular to working precision: `ok` is then a rounding accident on either side
        _aggregate("%s %d points" % (name, sizes[i]), (ok, H, B, eff), oracles[name].hb(sc, pose), with_ok=len(sc) >= min_pts)


# ---------------------------------------------------------------------------------------------- 3.5 points without a voxel
def _hostile_scan(small_world, pose):
    """scan2k with rows the table cannot hold (non-finite, keys beyond ±2^20 voxels, a coordinate beyond the int range) and rows that
    land within one voxel of the world's origin on either side of every axis. Returns (scan, rows that cannot contribute)."""
    s = np.array(small_world["scan2k"], copy=True)
    nan, inf = np.float32("nan"), np.float32("inf")
    bad = {5: (nan, 1.0, 2.0), 77: (1.0, nan, nan), 300: (inf, 0.0, 0.0), 301: (0.0, -inf, 1.0), 302: (inf, -inf, inf), 640: (3e7, 0.0, 0.0),
           641: (0.0, -3e7, 0.0), 642: (1.0, 2.0, 2.5e6), 1234: (5e9, 1.0, 1.0), 1235: (-5e9, -5e9, 1.0), 1999: (nan, nan, nan), 0: (-inf, 3e38, 1.0)}
    for r, v in bad.items():
        s[r] = v
    R = ref.rotation(pose).astype(np.float64)
    t = np.asarray(pose, dtype=np.float64)[4:]
    world = np.array([(x, y, z) for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)] +
                     [(-1.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, -1.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, -1.5), (0.5, 0.5, 1.5)])
    s[100:100 + len(world)] = ((world - t) @ R).astype(np.float32)  # Rᵀ·(w − t)
    return s, sorted(bad)


@pytest.mark.parametrize("name", ONE_EACH)
def test_points_the_table_cannot_hold_or_the_gate_must_refuse(gpu_ctx, api, locref, synth, small_world, name):
    """The target is the case's plus a blob of map points across the world's origin (the small world has none there)."""
    pose = small_world["true_pose"]
    s, bad = _hostile_scan(small_world, pose)
    ndt = cases.oracle_target(locref, synth, small_world, name, extra=cases.origin_blob())
    pp = cases.restate(ndt, name, s, pose)
    assert not pp["n_acc"][bad].any() and np.isnan(pp["res"][bad]).all()
    origin = pp["res"][100:114]
    assert (~np.isnan(origin)).all() and pp["n_acc"][100:114].sum() >= 14  # the cells touching 0 and their ±1 neighbours are all there
    _target(gpu_ctx, api, locref, synth, small_world, name, extra=cases.origin_blob())
    got = gpu_ctx.ndt_hb(s, pose)
    want = ndt.hb(s, pose)
    _aggregate(name + " hostile rows", got, want)
    assert cases.accepted_pairs(name, got[1], got[3]) == cases.accepted_pairs(name, want[1], want[3])
    if cases.CASES[name][0] == 1:
        assert got[3] == len(s)  # direct NDT counts every source point (ndt cpp:432)
    clean = gpu_ctx.ndt_hb(np.delete(s, bad, axis=0), pose)
    scale = np.abs(want[1]).max()
    print("%s: removing the %d rows changes H by %.2e of max|H|, B by %.2e" % (name, len(bad), np.abs(clean[1] - got[1]).max() / scale, np.abs(clean[2] - got[2]).max()))
    _hb_close(clean[1], clean[2], got[1], got[2])
    assert cases.accepted_pairs(name, clean[1], clean[3]) == cases.accepted_pairs(name, got[1], got[3])
    # the origin rows one by one, against the restatement: the double-width cells and the neighbours that straddle them
    rows = [gpu_ctx.ndt_hb(s[i:i + 1], pose) for i in range(100, 114)]
    near = ref.near_gate(pp["res"][100:114], cases.CASES[name][2], cases.GATE_REL)
    counts = np.array([cases.accepted_pairs(name, r[1], r[3]) for r in rows])
    assert np.array_equal(counts[~near], pp["n_acc"][100:114][~near])


# ---------------------------------------------------------------------------------------------- the gate at equality
def gate_world():
    """(map, scan, residual) of a world whose every (point, voxel) residual is one number, exactly, however it is grouped: the eight
    corners of a cube (a diagonal covariance: no Jacobi rotation, info = c·I with exact zeros off the diagonal) and source points half a
    metre from its centre along x, so res = (0.5·c)·0.5 = c / 4 — scalings by powers of two only. One point sits in the voxel itself, the
    other in its +x neighbour."""
    c = np.array([10.5, 10.5, 10.5])
    corners = np.array([(x, y, z) for x in (-0.25, 0.25) for y in (-0.25, 0.25) for z in (-0.25, 0.25)])
    return (c + corners).astype(np.float32), np.array([[10.0, 10.5, 10.5], [11.0, 10.5, 10.5]], np.float32)


@pytest.mark.parametrize("method", [1, 2])
def test_gate_keeps_a_residual_equal_to_the_threshold(gpu_ctx, api, locref, method):
    """`res > res_outlier_th` refuses (ndt cpp:417, :309): a residual EQUAL to the threshold is kept, one ulp above it is not."""
    m, s = gate_world()
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])  # under it the transform is exact
    probe = locref.Ndt(method=method)
    probe.set_target(m)
    keys, mu, info = probe.dump()
    assert len(keys) == 1 and tuple(keys[0]) == (10, 10, 10) and tuple(mu[0]) == (10.5, 10.5, 10.5)
    assert np.count_nonzero(info[0] - np.diag(np.diag(info[0]))) == 0
    res = info[0, 0, 0] / 4.0
    for th, pairs in ((res, 2), (np.nextafter(res, 0.0), 0), (np.nextafter(res, np.inf), 2)):
        ndt = locref.Ndt(method=method, res_outlier_th=th)
        ndt.set_target(m)
        if method == 2:
            gpu_ctx.ndt_set_target(m[:3], api.ndt_opts())  # a direct call starts the incremental voxel set afresh
        gpu_ctx.ndt_set_target(m, api.ndt_opts(method=method, res_outlier_th=th))
        ok_o, Ho, Bo, eff_o = ndt.hb(s, ident)
        ok_g, Hg, Bg, eff_g = gpu_ctx.ndt_hb(s, ident)
        print("method %d threshold %.17g (residual %.17g): accepted pairs GPU %g, oracle %g" % (method, th, res, Hg[3, 3] if method == 1 else eff_g, Ho[3, 3] if method == 1 else eff_o))
        assert eff_g == eff_o == (2 if method == 1 else pairs)
        assert Ho[3, 3] == (pairs if method == 1 else pairs * info[0, 0, 0])
        assert Hg[3, 3] == Hg[4, 4] == Hg[5, 5] == Ho[3, 3]  # exact on both sides: a count, or that count times the one information value
        _hb_close(Hg, Bg, Ho, Bo)


# ---------------------------------------------------------------------------------------------- 3.6 dropped and missing voxels
def test_dropped_and_missing_voxels(gpu_ctx, api, locref, small_world):
    """min_pts_in_voxel = 6: many voxels the map has are not in the table (ndt cpp:136-142), so a point's neighbours are a mix of kept,
    dropped and never-seen voxels. Then the det == 0 world: no voxel survives, H = 0, ok false on both sides."""
    s, pose = small_world["scan10k"], small_world["true_pose"]
    ndt = locref.Ndt(min_pts_in_voxel=6)
    ndt.set_target(small_world["map"])
    loose = locref.Ndt()
    loose.set_target(small_world["map"])
    assert 0 < ndt.num_voxels() < 0.9 * loose.num_voxels()
    gpu_ctx.ndt_set_target(small_world["map"], api.ndt_opts(min_pts_in_voxel=6))
    assert gpu_ctx.ndt_target_info()["num_voxels"] == ndt.num_voxels()
    got, want = gpu_ctx.ndt_hb(s, pose), ndt.hb(s, pose)
    _aggregate("min_pts_in_voxel 6", got, want)
    assert got[1][3, 3] == got[1][4, 4] == got[1][5, 5] == want[1][3, 3]
    rng = np.random.RandomState(11)
    m = (rng.rand(200, 3) * 100).astype(np.float32)
    ndt = locref.Ndt(min_pts_in_voxel=6)
    ndt.set_target(m)
    gpu_ctx.ndt_set_target(m, api.ndt_opts(min_pts_in_voxel=6))
    init = np.array([0, 0, 0, 1.0, 1, 2, 3])
    got, want = gpu_ctx.ndt_hb(m[:50], init), ndt.hb(m[:50], init)
    _aggregate("200-point random map", got, want)
    assert got[0] is False and want[0] is False and got[3] == 50


# ---------------------------------------------------------------------------------------------- 3.7 no side effects
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", ONE_EACH)
def test_an_evaluation_changes_nothing_an_alignment_depends_on(gpu_ctx, api, locref, synth, small_world, name, graph):
    s, init = small_world["scan10k"], small_world["init_pose"]
    scans = [small_world["scan2k"], s[::3], s[1::5]]
    inits = np.stack([init, init, small_world["true_pose"]])
    _target(gpu_ctx, api, locref, synth, small_world, name)
    b = gpu_ctx.batch(scans)
    try:
        gpu_ctx.graph_enable(graph)
        before = gpu_ctx.ndt_align(s, init)
        before_b = gpu_ctx.ndt_align_batch(b, inits)
        first = gpu_ctx.ndt_hb(s, small_world["true_pose"])
        hb = gpu_ctx.ndt_hb_batch(b, inits[::-1].copy())
        for _ in range(3):
            again = gpu_ctx.ndt_hb(s, small_world["true_pose"])
            assert again[1].tobytes() == first[1].tobytes() and again[2].tobytes() == first[2].tobytes() and again[0] == first[0] and again[3] == first[3]
            assert gpu_ctx.ndt_hb_batch(b, inits[::-1].copy()).tobytes() == hb.tobytes()
        after = gpu_ctx.ndt_align(s, init)
        after_b = gpu_ctx.ndt_align_batch(b, inits)
        assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1]
        assert after_b[0].tobytes() == before_b[0].tobytes() and after_b[1] == before_b[1]
        # an evaluation between a begin and its end is refused, by name, and the alignment ends as if nothing had happened
        gpu_ctx.ndt_align_batch_begin(b, inits)
        with pytest.raises(api.LocGpuError) as e:
            gpu_ctx.ndt_hb_batch(b, inits)
        assert e.value.code == -1 and "ndt_hb_batch" in str(e.value)
        ended = gpu_ctx.align_batch_end(b)
        assert ended[0].tobytes() == before_b[0].tobytes()
    finally:
        gpu_ctx.graph_enable(False)
        b.close()


def test_icp_evaluation_of_a_begun_batch_is_refused_by_name(gpu_ctx, api, small_world):
    """The refusal of a batch whose alignment has been begun comes first for the ICP callers of the shared evaluation as well."""
    s, init = small_world["scan2k"], small_world["init_pose"]
    opts = api.icp_opts(method=api.P2PLANE)
    gpu_ctx.icp_set_target(small_world["map"])
    b = gpu_ctx.batch([s, s[::2]])
    try:
        inits = np.stack([init, init])
        want = gpu_ctx.icp_align_batch(b, inits, opts)
        gpu_ctx.icp_align_batch_begin(b, inits, opts)
        with pytest.raises(api.LocGpuError) as e:
            gpu_ctx.icp_hb_batch(b, inits, opts)
        assert e.value.code == -1 and "icp_hb_batch" in str(e.value)
        got = gpu_ctx.align_batch_end(b)
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------- 3.8 errors
def test_errors_leave_the_context_usable(api, locref, small_world):
    L = api.lib()
    ctx = api.Context(0)
    try:
        s, pose = small_world["scan2k"], small_world["init_pose"]
        with pytest.raises(api.LocGpuError) as e:
            ctx.ndt_hb(s, pose)
        assert e.value.code == -3  # no NDT target
        b = ctx.batch([s])
        with pytest.raises(api.LocGpuError) as e:
            ctx.ndt_hb_batch(b, pose[None])
        assert e.value.code == -3
        ctx.ndt_set_target(small_world["map"])
        H, B, hb = np.zeros(36), np.zeros(6), np.zeros(44)
        p = np.ascontiguousarray(pose, dtype=np.float64)
        src = np.ascontiguousarray(s, dtype=np.float32)
        args = (src.ctypes.data, len(src), src.strides[0], p.ctypes.data, H.ctypes.data, B.ctypes.data, None, None)
        for hole in (0, 3, 4, 5):  # src, pose, H, B
            a = list(args)
            a[hole] = None
            assert L.locgpu_ndt_hb(ctx._h, *a) == -1, hole
        assert L.locgpu_ndt_hb(ctx._h, src.ctypes.data, 0, src.strides[0], p.ctypes.data, H.ctypes.data, B.ctypes.data, None, None) == -1  # empty source
        assert L.locgpu_ndt_hb_batch(ctx._h, None, p.ctypes.data, hb.ctypes.data) == -1
        assert L.locgpu_ndt_hb_batch(ctx._h, b._h, None, hb.ctypes.data) == -1
        assert L.locgpu_ndt_hb_batch(ctx._h, b._h, p.ctypes.data, None) == -1
        ndt = locref.Ndt()
        ndt.set_target(small_world["map"])
        want = ndt.hb(s, pose)
        _aggregate("after the refused calls", ctx.ndt_hb(s, pose), want)
        _aggregate("after the refused calls (batch)", _row(ctx.ndt_hb_batch(b, pose[None])[0]), want)
        b.close()
    finally:
        ctx.close()
