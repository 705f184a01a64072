"""LOAM on whole batches on the GPU: locgpu_batch_loam_extract (the feature picker on every scan of a batch, csrc/batch_loam.hip) and
locgpu_loam_align_batches (the matcher on two resident batches, csrc/loam_align.hip).

The picker is held to the single-cloud picker byte for byte. Every expected result is built two ways — the CPU oracle
(locref.loam_extract, ties ordered by ring position) and Cloud.loam_extract on the GPU — and the two must agree before the batch is
compared with them. Shapes are the smallest at which the kernels can go wrong (ring lengths either side of the skip threshold, of the
sector arithmetic, of the LDS sort's powers of two and of its capacity), not the workload.

The matcher is held to Loam.align_batch on the downloaded scans bit for bit, and the whole step — raw batch → loam_extract → in-place
preprocess of both feature batches → align_batches — to the oracle composition of tests/loam_ref.py at the bar of
tests/test_gpu_loam_stream.py (1e-8 m / rad). The world is that file's: the first 16 rings of synth.make_scan(i), maps = the picker's
unfiltered features of scan 0 at its true pose, leaf 0.5. Checked on the CPU with the oracle alone: maps of 1 920 / 18 837 points,
1 920 edges per scan (every sector full), filtered counts 1272 / 6194, 1237 / 6180, 1272 / 6283, 1262 / 6211, and four alignments
that end with status 0 through |dx| < 1e-3 after 7, 10, 13 and 13 evaluations."""
import numpy as np
import pytest

import loam_ref
from conftest import pose_delta

pytestmark = pytest.mark.gpu

INVALID = -1  # LOCGPU_ERR_INVALID
LEAF = 0.5
POSE_TOL = 1e-8  # metres and radians: the bar of tests/test_gpu_loam_stream.py for the same loop


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _xyzw(rows):
    """[n, 4] float32 with a fourth lane that tells points apart (the single-cloud picker carries it, the batch writes +0)."""
    c = np.zeros((len(rows), 4), np.float32)
    c[:, :3] = rows[:, :3]
    c[:, 3] = (np.arange(len(rows)) % 251).astype(np.float32)
    return c


def _rings_of(synth, scan_id, lengths, order=None):
    """A scan whose ring r has lengths[r] points: the first points of row r of synth.make_scan(scan_id) (rows of 1800; a longer ring runs
    on into the next rows, whose joints are as good an edge as any). Rings are laid down in `order`."""
    s = synth.make_scan(scan_id)
    parts, ring = [], []
    for r in (order if order is not None else range(len(lengths))):
        n = lengths[r]
        parts.append(s[r * 1800:r * 1800 + n, :3])
        assert len(parts[-1]) == n
        ring.append(np.full(n, r, np.uint8))
    return _xyzw(np.concatenate(parts)), np.concatenate(ring)


def _expected(api, locref, ctx, c, ring, num_scan):
    """x, y, z of (edge, surf) of one scan, built two ways that must agree: the CPU oracle and the single-cloud picker on the GPU."""
    if len(c):
        e_ref, s_ref = locref.loam_extract(c, ring, num_scan, order=locref.SORT_STABLE)
        cloud = api.Cloud(ctx, c)
    else:  # the oracle is not asked about nothing
        e_ref = s_ref = np.zeros((0, 4), np.float32)
        cloud = api.Cloud(ctx)
    edge, surf = cloud.loam_extract(ring, num_scan)
    e, s = edge.download(), surf.download()
    for x in (cloud, edge, surf):
        x.close()
    assert _same(e, e_ref) and _same(s, s_ref)
    return np.ascontiguousarray(e[:, :3]), np.ascontiguousarray(s[:, :3])


def _raw_batch(api, ctx, scans, max_points=None):
    b = ctx.batch_empty(len(scans), max_points if max_points is not None else max(max(len(s) for s in scans), 1))
    b.upload_async(scans)
    b.upload_wait()
    return b


def _scans_of(b):
    return [b.download_scan(s) for s in range(b.n_local)]


def _extract(api, ctx, scans, rings, num_scan, max_points=None, edge_cap=None, surf_cap=None):
    """(edge counts, surf counts, status, edge scans, surf scans) of one batched pass; the fourth lane must be +0 everywhere."""
    raw = _raw_batch(api, ctx, scans, max_points)
    longest = max(max(len(s) for s in scans), 1)
    edge = ctx.batch_empty(len(scans), edge_cap if edge_cap is not None else num_scan * 6 * 20)
    surf = ctx.batch_empty(len(scans), surf_cap if surf_cap is not None else longest)
    try:
        ne, ns, st = raw.loam_extract(rings, num_scan, edge, surf)
        e, s = _scans_of(edge), _scans_of(surf)
    finally:
        for b in (raw, edge, surf):
            b.close()
    for i in range(len(scans)):
        assert len(e[i]) == ne[i] and len(s[i]) == ns[i]
        assert not _bits(e[i][:, 3]).any() and not _bits(s[i][:, 3]).any()
    return ne, ns, st, [np.ascontiguousarray(x[:, :3]) for x in e], [np.ascontiguousarray(x[:, :3]) for x in s]


# ---- 1. the picker's own edges -------------------------------------------------------------------------------------------------
def test_ragged_batch_across_the_pickers_own_edges(api, gpu_ctx, locref, synth):
    """num_scan = 3. Ring lengths: 0, 130 | 131 (skip threshold); 136 | 137 ((size − 10) / 6 = 21 with remainders 0 | 1 in sector 5);
    778 (sectors of 127 → a power of two of 128, one compaction round); 1552 (sectors of 256 / 257: two rounds); 12 298 (a sector of
    exactly 2048, the LDS sort's capacity). Beside them an empty scan, a scan whose only points carry ring 3 (ignored), and a scan
    delivered column-major with returns missing and one ring thinned below the threshold."""
    scans, rings = [], []
    for scan_id, lengths, order in ((1, (0, 130, 131), (2, 1)), (2, (136, 137, 778), (1, 2, 0)), (3, (1552, 12298, 0), (1, 0))):
        c, r = _rings_of(synth, scan_id, lengths, order)
        scans.append(c)
        rings.append(r)
    scans.append(np.zeros((0, 4), np.float32))
    rings.append(np.zeros(0, np.uint8))
    c, r = _rings_of(synth, 4, (0, 0, 0, 300), (3,))
    scans.append(c)
    rings.append(r)
    # test_loam_extract_interleaved_input_and_partial_rings (tests/test_gpu_loam_features.py) cut to three rings: ring 1 keeps 1 in 16
    c, r = _rings_of(synth, 9, (1800, 1800, 1800))
    perm = np.argsort(np.arange(len(c)) % 1800, kind="stable")
    c, r = c[perm], r[perm]
    keep = np.ones(len(c), bool)
    keep[::13] = False
    keep[(r == 1) & (np.arange(len(c)) % 16 != 0)] = False
    scans.append(np.ascontiguousarray(c[keep]))
    rings.append(np.ascontiguousarray(r[keep]))
    assert 0 < int((rings[-1] == 1).sum()) < 131

    want = [_expected(api, locref, gpu_ctx, c, r, 3) for c, r in zip(scans, rings)]
    ne, ns, st, e, s = _extract(api, gpu_ctx, scans, rings, 3)
    print("edge counts", ne.tolist(), "surf counts", ns.tolist(), "status", st.tolist())
    assert not st.any()
    for i, (we, ws) in enumerate(want):
        assert _same(e[i], we) and _same(s[i], ws), i
    assert ne[3] == ns[3] == 0 and ne[4] == ns[4] == 0
    assert sum(1 for w in want if len(w[0]) > 0) >= 3


# ---- 2. independence of the batch ----------------------------------------------------------------------------------------------
def test_a_scans_bytes_do_not_depend_on_the_batch(api, gpu_ctx, locref, synth):
    """Five scans of 13 rings (n_scans · num_scan = 65: not a power of two, and one more sort bit than 64 needs) as batches of 1, 3 and
    5, at different positions, with max_points_per_scan at the largest count and well above it."""
    rng = np.random.default_rng(20)
    scans, rings = [], []
    for k in range(5):
        lengths = [int(v) for v in rng.integers(120, 420, 13)]
        lengths[k] = 131 + k
        order = [int(v) for v in rng.permutation(13)]
        c, r = _rings_of(synth, 10 + k, lengths, order)
        scans.append(c)
        rings.append(r)
    want = [_expected(api, locref, gpu_ctx, c, r, 13) for c, r in zip(scans, rings)]
    assert all(len(w[0]) > 0 and len(w[1]) > 0 for w in want)
    longest = max(len(c) for c in scans)
    for pick, max_points in (((0,), None), ((3,), 3 * longest), ((4, 0, 2), None), ((1, 3, 4), 2 * longest + 77), ((0, 1, 2, 3, 4), None),
                             ((4, 3, 2, 1, 0), longest + 1000)):
        ne, ns, st, e, s = _extract(api, gpu_ctx, [scans[i] for i in pick], [rings[i] for i in pick], 13, max_points=max_points,
                                    surf_cap=max_points)
        assert not st.any()
        for at, i in enumerate(pick):
            assert _same(e[at], want[i][0]) and _same(s[at], want[i][1]), (pick, max_points, i)


# ---- 3. ties and flat rings ----------------------------------------------------------------------------------------------------
def test_ties_and_flat_rings_in_one_batch(api, gpu_ctx, locref, synth):
    """The polygon (equal curvatures everywhere) and the circle (no curvature above 0.1) of test_loam_extract_ties_and_flat_rings beside
    a synthetic scan."""
    th = np.linspace(0, 2 * np.pi, 720, endpoint=False)
    sq = np.stack([np.clip(8 * np.cos(th), -5, 5), np.clip(8 * np.sin(th), -5, 5), np.zeros_like(th), np.arange(720) % 200], 1).astype(np.float32)
    polygon = np.concatenate([sq, sq + np.array([0, 0, 1, 0], np.float32)])
    flat = np.stack([10 * np.cos(th), 10 * np.sin(th), np.zeros_like(th), np.arange(720)], 1).astype(np.float32)
    c, r = _rings_of(synth, 5, (1800, 1800))
    scans = [polygon, c, flat]
    rings = [np.repeat(np.arange(2), 720).astype(np.uint8), r, np.zeros(720, np.uint8)]
    want = [_expected(api, locref, gpu_ctx, c, r, 2) for c, r in zip(scans, rings)]
    ne, ns, st, e, s = _extract(api, gpu_ctx, scans, rings, 2)
    for i, (we, ws) in enumerate(want):
        assert _same(e[i], we) and _same(s[i], ws), i
    assert ne[0] > 0 and ne[1] > 0 and ne[2] == 0 and ns[2] == 710 - 6


# ---- 4. capacity and refusals --------------------------------------------------------------------------------------------------
def _filled(ctx, n_scans, cap, seed):
    """A destination with known content: (batch, its scans as downloaded)."""
    rng = np.random.default_rng(seed)
    scans = [rng.normal(size=(int(rng.integers(0, cap + 1)), 4)).astype(np.float32) for _ in range(n_scans)]
    b = ctx.batch_empty(n_scans, cap)
    b.upload_async(scans)
    b.upload_wait()
    return b, _scans_of(b)


def _refused(api, raw, rings, num_scan, edge, surf, before_e, before_s):
    with pytest.raises(api.LocGpuError) as err:
        raw.loam_extract(rings, num_scan, edge, surf)
    assert err.value.code == INVALID and str(err.value)
    for b, before in ((edge, before_e), (surf, before_s)):
        after = _scans_of(b)
        assert len(after) == len(before) and all(_same(x, y) for x, y in zip(after, before))
    return err.value


def test_capacity_and_refusals(api, gpu_ctx, locref, synth):
    scans, rings = [], []
    for k in range(3):
        c, r = _rings_of(synth, 20 + k, (200 + 7 * k, 150, 131))
        scans.append(c)
        rings.append(r)
    want = [_expected(api, locref, gpu_ctx, c, r, 3) for c, r in zip(scans, rings)]
    need_e, need_s = max(len(w[0]) for w in want), max(len(w[1]) for w in want)
    assert need_e > 1 and need_s > 1
    raw = _raw_batch(api, gpu_ctx, scans)
    made = [raw]
    try:
        # a destination one point too small: the needed counts come back, both destinations stay, a second call with room succeeds
        for e_cap, s_cap in ((need_e - 1, need_s), (need_e, need_s - 1)):
            edge, be = _filled(gpu_ctx, 3, e_cap, 1)
            surf, bs = _filled(gpu_ctx, 3, s_cap, 2)
            made += [edge, surf]
            err = _refused(api, raw, rings, 3, edge, surf, be, bs)
            assert err.edge_counts.tolist() == [len(w[0]) for w in want] and err.surf_counts.tolist() == [len(w[1]) for w in want]
            assert not err.status.any()
        edge, be = _filled(gpu_ctx, 3, need_e, 3)
        surf, bs = _filled(gpu_ctx, 3, need_s, 4)
        made += [edge, surf]
        ne, ns, st = raw.loam_extract(rings, 3, edge, surf)
        for i, (e, s) in enumerate(zip(_scans_of(edge), _scans_of(surf))):
            assert _same(np.ascontiguousarray(e[:, :3]), want[i][0]) and _same(np.ascontiguousarray(s[:, :3]), want[i][1]), i
        be, bs = _scans_of(edge), _scans_of(surf)
        # num_scan out of range, edge is surf, a NULL ring array for a scan with points
        for bad in (0, 257):
            _refused(api, raw, rings, bad, edge, surf, be, bs)
        _refused(api, raw, rings, 3, edge, edge, be, be)
        _refused(api, raw, [rings[0], None, rings[2]], 3, edge, surf, be, bs)
        # a 13 000-point ring in scan 2 of 3: the single-cloud picker's loud refusal, per scan
        long_scans = [scans[0], scans[1], np.random.default_rng(1).normal(size=(13000, 4)).astype(np.float32)]
        long_rings = [rings[0], rings[1], np.zeros(13000, np.uint8)]
        long_raw = _raw_batch(api, gpu_ctx, long_scans)
        made.append(long_raw)
        big = gpu_ctx.batch_empty(3, 13000)
        made.append(big)
        err = _refused(api, long_raw, long_rings, 3, edge, big, be, _scans_of(big))
        assert err.status.tolist() == [0, 0, 1] and "scan 2" in str(err)
        # batches of two contexts, a shared-source batch
        other = api.Context(0)
        try:
            foreign = other.batch_empty(3, need_s)
            with pytest.raises(api.LocGpuError) as e2:
                raw.loam_extract(rings, 3, edge, foreign)
            assert e2.value.code == INVALID
            foreign.close()
        finally:
            other.close()
        shared = gpu_ctx.batch_shared(scans[0], 3)
        made.append(shared)
        with pytest.raises(api.LocGpuError) as e3:
            raw.loam_extract(rings, 3, edge, shared)
        assert e3.value.code == INVALID
        be2, bs2 = _scans_of(edge), _scans_of(surf)
        assert all(_same(x, y) for x, y in zip(be2, be)) and all(_same(x, y) for x, y in zip(bs2, bs))
    finally:
        for b in made:
            b.close()
    # n_scans · num_scan above 65535: refused before anything is allocated
    tiny = [gpu_ctx.batch_empty(300, 1) for _ in range(3)]
    try:
        with pytest.raises(api.LocGpuError) as err:
            tiny[0].loam_extract([None] * 300, 256, tiny[1], tiny[2])
        assert err.value.code == INVALID and "65535" in str(err.value)
    finally:
        for b in tiny:
            b.close()


# ---- 5–9. Lio's step on a batch ------------------------------------------------------------------------------------------------
N_PTS, NUM_SCAN, RING_LEN = 28800, 16, 1800
SCAN_IDS = (1, 2, 3, 4)
FILTERED = ((1272, 6194), (1237, 6180), (1272, 6283), (1262, 6211))
ITERATIONS = (7, 10, 13, 13)


def _raw_scan(synth, i):
    s = synth.make_scan(i)[:N_PTS]
    assert len(s) == N_PTS
    return _xyzw(s), (np.arange(N_PTS) // RING_LEN).astype(np.uint8)


@pytest.fixture(scope="module")
def world(locref, synth):
    """CPU data computed once and never modified: the maps, the raw scans, the oracle's filtered features and alignments."""
    c0, r0 = _raw_scan(synth, 0)
    e0, s0 = locref.loam_extract(c0, r0, NUM_SCAN, order=locref.SORT_STABLE)
    truth0 = synth.make_pose(0)[0]
    edge_map, surf_map = locref.transform_cloud_f64(truth0, e0), locref.transform_cloud_f64(truth0, s0)
    assert (len(edge_map), len(surf_map)) == (1920, 18837)
    oracle = loam_ref.LoamOracle(locref, edge_map[:, :3], surf_map[:, :3])
    w = dict(edge_map=edge_map, surf_map=surf_map, raw=[], rings=[], init=[], edge=[], surf=[], want=[])
    for i in SCAN_IDS:
        c, r = _raw_scan(synth, i)
        e, s = locref.loam_extract(c, r, NUM_SCAN, order=locref.SORT_STABLE)
        assert len(e) == 1920  # every sector full
        e, s = (locref.voxel_grid(x, True, LEAF, order=locref.SORT_STABLE) for x in (e, s))
        init = np.array(synth.make_pose(i)[1], dtype=np.float64)
        w["raw"].append(c)
        w["rings"].append(r)
        w["init"].append(init)
        w["edge"].append(np.ascontiguousarray(e[:, :3]))
        w["surf"].append(np.ascontiguousarray(s[:, :3]))
        w["want"].append(oracle.scan_match(e[:, :3], s[:, :3], init))
    w["init"] = np.array(w["init"])
    assert tuple((len(e), len(s)) for e, s in zip(w["edge"], w["surf"])) == FILTERED
    assert tuple(x["iterations"] for x in w["want"]) == ITERATIONS and all(x["status"] == 0 and x["converged"] for x in w["want"])
    return w


def _features(ctx, raws, rings):
    """raw batch → loam_extract → in-place preprocess of both feature batches: (edge batch, surf batch, picked edge counts)."""
    raw = _raw_batch(None, ctx, raws, N_PTS)
    edge, surf = ctx.batch_empty(len(raws), NUM_SCAN * 6 * 20), ctx.batch_empty(len(raws), N_PTS)
    ne, ns, st = raw.loam_extract(rings, NUM_SCAN, edge, surf)
    raw.close()
    assert not st.any()
    edge.preprocess(LEAF)
    surf.preprocess(LEAF)
    return edge, surf, ne


def _handle(api, world, **opts):
    h = api.Loam(api.loam_opts(**opts))
    h.set_target(world["edge_map"] if opts.get("use_edge_points", 1) else None, world["surf_map"] if opts.get("use_surf_points", 1) else None)
    return h


@pytest.fixture(scope="module")
def step(api, gpu_ctx, world):
    """The step of test 5, run once: feature batches (kept alive for the tests that reuse them), poses and stats."""
    edge, surf, picked = _features(gpu_ctx, world["raw"], world["rings"])
    h = _handle(api, world)
    poses, stats = h.align_batches(edge, surf, world["init"])
    yield dict(edge=edge, surf=surf, picked=picked, h=h, poses=poses, stats=stats)
    h.close()
    edge.close()
    surf.close()


def test_lios_step_on_a_batch_against_the_oracle(api, gpu_ctx, world, step):
    edge, surf, h = step["edge"], step["surf"], step["h"]
    assert step["picked"].tolist() == [1920] * 4
    e, s = _scans_of(edge), _scans_of(surf)
    assert tuple((len(a), len(b)) for a, b in zip(e, s)) == FILTERED
    for i in range(4):
        assert _same(np.ascontiguousarray(e[i][:, :3]), world["edge"][i]) and _same(np.ascontiguousarray(s[i][:, :3]), world["surf"][i]), i
    poses_h, stats_h = h.align_batch(e, s, world["init"])
    assert _same(step["poses"], poses_h) and step["stats"] == stats_h
    # align_batches read the batches, it did not change them
    assert all(_same(a, b) for a, b in zip(_scans_of(edge) + _scans_of(surf), e + s))
    for i, st in enumerate(step["stats"]):
        dt, dr = pose_delta(step["poses"][i], world["want"][i]["pose"])
        print("scan %d: iterations %d, status %d, dt %.3e m, dr %.3e rad" % (SCAN_IDS[i], st["iterations"], st["status"], dt, dr))
        assert st["status"] == 0 and st["iterations"] == ITERATIONS[i], (i, st)
        assert dt < POSE_TOL and dr < POSE_TOL, (i, dt, dr)


def test_a_failing_scan_leaves_the_others_alone(api, gpu_ctx, world, step):
    """Scan 2 replaced by 4 rings × 100 points: no ring reaches 131 points, no features, the surface class reports false first."""
    raws, rings = list(world["raw"]), list(world["rings"])
    raws[1] = np.ascontiguousarray(raws[1][:400])
    rings[1] = (np.arange(400) // 100).astype(np.uint8)
    edge, surf, picked = _features(gpu_ctx, raws, rings)
    try:
        assert picked[1] == 0 and len(surf.download_scan(1)) == 0
        poses, stats = step["h"].align_batches(edge, surf, world["init"])
        assert stats[1]["status"] == 3 and _same(poses[1], world["init"][1])
        for i in (0, 2, 3):
            assert _same(poses[i], step["poses"][i]) and stats[i] == step["stats"][i], i
    finally:
        edge.close()
        surf.close()


@pytest.mark.parametrize("off", ["edge", "surf"])
def test_a_switched_off_class_takes_no_batch(api, world, step, off):
    h = _handle(api, world, **{"use_%s_points" % off: 0})
    try:
        edge = None if off == "edge" else step["edge"]
        surf = None if off == "surf" else step["surf"]
        poses, stats = h.align_batches(edge, surf, world["init"])
        poses_h, stats_h = h.align_batch(None if off == "edge" else _scans_of(edge), None if off == "surf" else _scans_of(surf), world["init"])
        assert _same(poses, poses_h) and stats == stats_h
        assert all(st["iterations"] >= 1 for st in stats)
    finally:
        h.close()


def test_fitness_resident_is_refused_after_align_batches(api, world, step):
    h = step["h"]
    pose, st, _ = h.scan_match(world["edge"][0], world["surf"][0], world["init"][0])
    assert len(h.fitness_resident(pose)) == 2  # a single-scan call leaves its scans
    h.align_batches(step["edge"], step["surf"], world["init"])
    with pytest.raises(api.LocGpuError) as err:
        h.fitness_resident(pose)
    assert err.value.code == INVALID


def test_feature_batches_of_another_context_align_alike(api, world, step):
    front = api.Context(0)
    try:
        edge, surf, _ = _features(front, world["raw"], world["rings"])
        poses, stats = step["h"].align_batches(edge, surf, world["init"])
        assert _same(poses, step["poses"]) and stats == step["stats"]
        edge.close()
        surf.close()
    finally:
        front.close()
