"""Range-image ingest on the GPU (csrc/range_ingest.hip): locgpu_batch_upload_ranges, locgpu_batch_download_rings,
locgpu_batch_loam_extract_resident and locgpu_cloud_upload_ranges against the numpy float32 restatement of the definition
(tests/range_image_ref.py), byte for byte.

Sensor A: 4 rings × 300 columns (1200 cells: one tile of the kernels, zero runs across 256, 512, 768 and 1024). Sensor B: 16 × 64 with
per-laser azimuth tables. Beyond the two the issue names, two shapes at which the kernels take other paths: sensor C, 5 × 1231 = 6155
cells — four tiles of 2048 cells, the last one partial, and 6155 = 8 · 769 + 3, so the last 16-byte load of a scan holds three cells
and five of padding; sensor D, 256 × 2100 = 537 600 cells — 263 tiles, more than the 256 the per-scan offsets kernel sums per trip,
and ring bytes up to 255. Four images per sensor: all zero; all hit, counts up to 65 535; about 30 % zeros in runs across every
multiple of 256 cells (returns below min_range mixed in); every return below min_range."""
import ctypes

import numpy as np
import pytest

import range_image_ref as ref

pytestmark = pytest.mark.gpu

INVALID = -1  # LOCGPU_ERR_INVALID
SCALE, MIN_RANGE = 0.002, 4.0  # 2 mm per count: 65 535 counts = 131 m; 4 m = 2000 counts
LEAF = 0.5


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _tables(synth, n_rings, n_cols, per_ring):
    cos_el, sin_el, cos_az, sin_az = synth.sensor_tables(n_rings, n_cols)
    if per_ring:  # laser g fires 0.37 g degrees behind laser 0
        az = 2.0 * np.pi * np.arange(n_cols)[None, :] / n_cols + np.deg2rad(0.37) * np.arange(n_rings)[:, None]
        cos_az, sin_az = np.cos(az).astype(np.float32), np.sin(az).astype(np.float32)
    return cos_el, sin_el, cos_az, sin_az


def _images(cells, seed):
    rng = np.random.default_rng(seed)
    zero = np.zeros(cells, np.uint16)
    hit = rng.integers(2100, 65536, cells).astype(np.uint16)
    hit[:: max(cells // 7, 1)] = 65535
    holes = rng.integers(2100, 65536, cells).astype(np.uint16)
    near = rng.random(cells) < 0.05
    holes[near] = rng.integers(1, 1900, int(near.sum())).astype(np.uint16)
    gone = np.zeros(cells, bool)
    gone[:int(cells * 0.045)] = True
    for m in range(256, cells + 256, 256):  # a run across every multiple of 256 (and so of 1024)
        gone[max(m - 38, 0):min(m + 39, cells)] = True
    holes[gone] = 0
    assert 0.25 < gone.mean() < 0.36
    short = rng.integers(1, 1900, cells).astype(np.uint16)
    return [zero, hit, holes, short]


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(api, synth, ctx):
    """Per sensor: the model, its resident form, four images and the restatement's (points, rings) of each. Computed once, never modified."""
    w = {}
    for name, n_rings, n_cols, per_ring in (("A", 4, 300, False), ("B", 16, 64, True), ("C", 5, 1231, False), ("D", 256, 2100, False)):
        model = api.SensorModel(n_rings, n_cols, SCALE, MIN_RANGE, *_tables(synth, n_rings, n_cols, per_ring))
        images = _images(model.cells, 11 + n_rings)
        want = [ref.decode(model, im) for im in images]
        assert len(want[0][0]) == 0 and len(want[1][0]) == model.cells and 0 < len(want[2][0]) < 0.75 * model.cells and len(want[3][0]) == 0
        w[name] = dict(model=model, sensor=api.Sensor(ctx, model), images=images, want=want)
    yield w
    for v in w.values():
        v["sensor"].close()


def _state(b):
    """Everything a batch with resident rings holds, as downloaded."""
    return [(b.download_scan(s), b.download_rings(s)) for s in range(b.n_local)]


def _check(b, counts, want, pick):
    got = _state(b)
    for at, i in enumerate(pick):
        pts, rings = got[at]
        assert counts[at] == len(want[i][0]) == len(pts), (pick, i)
        assert _same(pts, want[i][0]) and not _bits(pts[:, 3]).any(), (pick, i)
        assert rings.dtype == np.uint8 and np.array_equal(rings, want[i][1]), (pick, i)


# ---- 1. the decode against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_decode_equals_the_restatement_byte_for_byte(ctx, world, name):
    v = world[name]
    cells, want = v["model"].cells, v["want"]
    picks = [(0, 1, 2, 3), (0, 1, 2, 3), (3, 2, 1, 0), (0,), (1,), (2,), (3,)] if name != "D" else [(2, 1), (2, 1), (1,), (2,)]
    for pick in picks:  # the same batch twice (a second run), another order, every scan alone
        b = ctx.batch_empty(len(pick), cells)
        try:
            counts = b.upload_ranges(v["sensor"], [v["images"][i] for i in pick])
            print(name, pick, counts.tolist())
            _check(b, counts, want, pick)
        finally:
            b.close()
    # a batch that is larger than the scans need, filled twice: the second call replaces the first
    b = ctx.batch_empty(2, cells + 77)
    try:
        b.upload_ranges(v["sensor"], [v["images"][1], v["images"][2]])
        counts = b.upload_ranges(v["sensor"], [v["images"][2], v["images"][0]])
        _check(b, counts, want, (2, 0))
    finally:
        b.close()


def test_ingest_times_are_reported_while_profiling(ctx, world):
    v = world["C"]
    b = ctx.batch_empty(4, v["model"].cells)
    try:
        ctx.profile_enable(True)
        b.upload_ranges(v["sensor"], v["images"])
        copy_ms, kernel_ms = ctx.range_ingest_times()
        assert 0 < copy_ms < 1e3 and 0 < kernel_ms < 1e3
    finally:
        ctx.profile_enable(False)
        b.close()


# ---- 2. what follows the ingest ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_preprocess_and_alignment_downstream(api, synth, ctx, world, name):
    v = world[name]
    cells = v["model"].cells
    raw_r, raw_h = ctx.batch_empty(4, cells), ctx.batch_empty(4, cells)
    flt_r, flt_h = ctx.batch_empty(4, cells), ctx.batch_empty(4, cells)
    try:
        raw_r.upload_ranges(v["sensor"], v["images"])
        raw_h.upload_async([w[0] for w in v["want"]])
        raw_h.upload_wait()
        cr, sr = raw_r.preprocess(LEAF, out=flt_r)
        ch, sh = raw_h.preprocess(LEAF, out=flt_h)
        assert cr.tolist() == ch.tolist() and sr.tolist() == sh.tolist() and cr[1] > 0 and cr[0] == 0
        for s in range(4):
            assert _same(flt_r.download_scan(s), flt_h.download_scan(s)), s
        ctx.icp_set_target(synth.make_local_map(2000, 3, half=40.0))
        init = np.array([synth.make_pose(3)[1]] * 4)
        opts = api.icp_opts(method=api.P2P, max_iteration=5)
        poses_r, stats_r = ctx.icp_align_batch(flt_r, init, opts)
        poses_h, stats_h = ctx.icp_align_batch(flt_h, init, opts)
        assert _same(poses_r, poses_h) and stats_r == stats_h
        assert any(st["iterations"] >= 1 for st in stats_r)
    finally:
        for b in (raw_r, raw_h, flt_r, flt_h):
            b.close()


# ---- 3. capacity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_capacity_refusal_leaves_the_batch_as_it_was(api, ctx, world, name):
    v = world[name]
    need = [len(w[0]) for w in v["want"]]
    largest = max(need)
    few = []
    for im in v["images"]:  # images with at most 100 returns: they fit the small batch
        a = im.copy()
        a[100:] = 0
        few.append(a)
    b = ctx.batch_empty(4, largest - 1)
    try:
        before_counts = b.upload_ranges(v["sensor"], few)
        assert before_counts[1] == 100
        before = _state(b)
        with pytest.raises(api.LocGpuError) as err:
            b.upload_ranges(v["sensor"], v["images"])
        assert err.value.code == INVALID and str(largest) in str(err.value)
        assert err.value.counts.tolist() == need
        after = _state(b)
        assert len(after) == len(before)
        for (p0, r0), (p1, r1) in zip(before, after):
            assert _same(p0, p1) and np.array_equal(r0, r1)
    finally:
        b.close()
    b = ctx.batch_empty(4, largest)  # exactly enough
    try:
        counts = b.upload_ranges(v["sensor"], v["images"])
        _check(b, counts, v["want"], (0, 1, 2, 3))
    finally:
        b.close()


# ---- 4 / 5. LOAM downstream ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loam_world(api, synth, ctx, world):
    """Sensor A images for the picker: a synthetic scan (smooth rings), the all-hit image, the image with holes, and the synthetic
    scan with ring 2 thinned to 100 returns (below the picker's 131). The restatement's clouds and rings, and the batched picker's
    result from HOST ring arrays."""
    v = world["A"]
    model = v["model"]
    scan = synth.make_range_image(3, model).reshape(-1)
    thin = scan.copy()
    thin[2 * 300 + 100:3 * 300] = 0
    images = [scan, v["images"][1], v["images"][2], thin]
    want = [ref.decode(model, im) for im in images]
    per_ring = [np.bincount(w[1], minlength=4).tolist() for w in want]
    assert all(n >= 131 for n in per_ring[0]) and all(n >= 131 for n in per_ring[1]) and 0 < per_ring[3][2] < 131
    raw, edge, surf = ctx.batch_empty(4, 1200), ctx.batch_empty(4, 4 * 6 * 20), ctx.batch_empty(4, 1200)
    raw.upload_async([w[0] for w in want])
    raw.upload_wait()
    ne, ns, st = raw.loam_extract([w[1] for w in want], 4, edge, surf)
    host = dict(ne=ne, ns=ns, st=st, edge=[edge.download_scan(s) for s in range(4)], surf=[surf.download_scan(s) for s in range(4)])
    assert not st.any() and ne[0] > 0 and ns[0] > 0 and ns[3] > 0
    for b in (raw, edge, surf):
        b.close()
    return dict(images=images, want=want, host=host)


def test_loam_extract_resident_equals_the_host_ring_form(api, ctx, world, loam_world):
    sensor, host = world["A"]["sensor"], loam_world["host"]
    raw, edge, surf = ctx.batch_empty(4, 1200), ctx.batch_empty(4, 4 * 6 * 20), ctx.batch_empty(4, 1200)
    plain = ctx.batch_empty(4, 1200)
    try:
        raw.upload_ranges(sensor, loam_world["images"])
        ne, ns, st = raw.loam_extract_resident(4, edge, surf)
        assert ne.tolist() == host["ne"].tolist() and ns.tolist() == host["ns"].tolist() and st.tolist() == host["st"].tolist()
        for s in range(4):
            assert _same(edge.download_scan(s), host["edge"][s]) and _same(surf.download_scan(s), host["surf"][s]), s
        # the same batch with its rings handed in from the host: locgpu_batch_loam_extract is unchanged
        ne2, ns2, _ = raw.loam_extract([w[1] for w in loam_world["want"]], 4, edge, surf)
        assert ne2.tolist() == ne.tolist() and ns2.tolist() == ns.tolist()
        # the destinations' own rings are not the features' rings
        for b in (edge, surf):
            with pytest.raises(api.LocGpuError) as err:
                b.download_rings(0)
            assert err.value.code == INVALID
        # refused: a batch filled by upload_async ...
        plain.upload_async([w[0] for w in loam_world["want"]])
        plain.upload_wait()
        keep_e = [edge.download_scan(s) for s in range(4)]
        with pytest.raises(api.LocGpuError) as err:
            plain.loam_extract_resident(4, edge, surf)
        assert err.value.code == INVALID and "resident rings" in str(err.value)
        # ... a batch whose rings a later upload dropped, or a preprocess into it
        raw.upload_async([w[0] for w in loam_world["want"]])
        raw.upload_wait()
        with pytest.raises(api.LocGpuError) as err:
            raw.loam_extract_resident(4, edge, surf)
        assert err.value.code == INVALID
        raw.upload_ranges(sensor, loam_world["images"])
        assert len(raw.download_rings(1)) == 1200
        raw.preprocess(LEAF)
        for call in (lambda: raw.loam_extract_resident(4, edge, surf), lambda: raw.download_rings(1)):
            with pytest.raises(api.LocGpuError) as err:
                call()
            assert err.value.code == INVALID
        assert all(_same(edge.download_scan(s), keep_e[s]) for s in range(4))
        # the limits of locgpu_batch_loam_extract hold
        raw.upload_ranges(sensor, loam_world["images"])
        for bad in (0, 257):
            with pytest.raises(api.LocGpuError) as err:
                raw.loam_extract_resident(bad, edge, surf)
            assert err.value.code == INVALID
    finally:
        for b in (raw, edge, surf, plain):
            b.close()


def test_cloud_upload_ranges_equals_the_batch_form(api, ctx, world, loam_world):
    sensor, host = world["A"]["sensor"], loam_world["host"]
    cloud = api.Cloud(ctx)
    try:
        for s, (pts, rings) in enumerate(loam_world["want"]):
            got_rings = cloud.upload_ranges(sensor, loam_world["images"][s])
            assert cloud.info == (len(pts), True)
            assert _same(cloud.download(), pts) and np.array_equal(got_rings, rings), s
            edge, surf = cloud.loam_extract(got_rings, 4)
            assert _same(edge.download(), host["edge"][s]) and _same(surf.download(), host["surf"][s]), s
            edge.close()
            surf.close()
        assert cloud.upload_ranges(sensor, world["A"]["images"][0], with_rings=False) is None and len(cloud) == 0
    finally:
        cloud.close()
    # more than one tile, a tail of three cells
    c = api.Cloud(ctx)
    try:
        for s in (2, 1, 3):
            rings = c.upload_ranges(world["C"]["sensor"], world["C"]["images"][s])
            assert _same(c.download(), world["C"]["want"][s][0]) and np.array_equal(rings, world["C"]["want"][s][1]), s
    finally:
        c.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(api, ctx, world):
    L = api.lib()
    v = world["A"]
    base = v["model"]

    def create(**over):
        m = base.c_struct()
        for k, val in over.items():
            setattr(m, k, val)
        h = ctypes.c_void_p()
        rc = L.locgpu_sensor_create(ctx._h, ctypes.byref(m), ctypes.byref(h))
        text = L.locgpu_last_error(ctx._h).decode()
        if rc == 0:
            L.locgpu_sensor_destroy(h)
        return rc, text

    assert create()[0] == 0
    for over in (dict(n_rings=0), dict(n_rings=257), dict(n_cols=0), dict(n_cols=12289), dict(range_scale=0.0), dict(range_scale=-0.002),
                 dict(range_scale=float("nan")), dict(range_scale=float("inf")), dict(min_range=-1.0), dict(min_range=float("nan")), dict(az_per_ring=2),
                 dict(cos_el=None), dict(sin_el=None), dict(cos_az=None), dict(sin_az=None)):
        rc, text = create(**over)
        assert rc == INVALID and text.startswith("sensor_create"), (over, rc, text)
    assert create(min_range=0.0)[0] == 0

    def refused(call):
        with pytest.raises(api.LocGpuError) as err:
            call()
        assert err.value.code == INVALID and len(str(err.value)) > 20
        return str(err.value)

    scan = v["want"][1][0]
    images = v["images"]
    sharded = api.Batch(ctx, [scan] * 4, first=0, n_total=4)
    shared = ctx.batch_shared(scan, 4)
    plain = ctx.batch_empty(4, 1200)
    other = api.Context(0)
    try:
        refused(lambda: sharded.upload_ranges(v["sensor"], images))
        refused(lambda: shared.upload_ranges(v["sensor"], images))
        foreign = api.Sensor(other, base)
        assert "another context" in refused(lambda: plain.upload_ranges(foreign, images))
        cloud = api.Cloud(ctx)
        assert "another context" in refused(lambda: cloud.upload_ranges(foreign, images[1]))
        cloud.close()
        foreign.close()
        # a NULL image, NULL images, a NULL sensor
        ptrs = (ctypes.c_void_p * 4)(images[0].ctypes.data, None, images[2].ctypes.data, images[3].ctypes.data)
        assert L.locgpu_batch_upload_ranges(plain._h, v["sensor"]._h, ptrs, None) == INVALID and b"images[1]" in L.locgpu_last_error(ctx._h)
        assert L.locgpu_batch_upload_ranges(plain._h, v["sensor"]._h, None, None) == INVALID
        assert L.locgpu_batch_upload_ranges(plain._h, None, ptrs, None) == INVALID
        # no rings yet
        refused(lambda: plain.download_rings(0))
        # an alignment begun and not ended
        plain.upload_ranges(v["sensor"], images)
        before = _state(plain)
        ctx.icp_set_target(scan[:, :3])
        ctx.icp_align_batch_begin(plain, np.array([[0, 0, 0, 1, 0, 0, 0.0]] * 4), api.icp_opts(method=api.P2P, max_iteration=2))
        try:
            assert "begun" in refused(lambda: plain.upload_ranges(v["sensor"], images))
        finally:
            ctx.align_batch_end(plain)
        after = _state(plain)
        assert all(_same(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before, after))
        refused(lambda: plain.download_rings(4))
    finally:
        other.close()
        for b in (sharded, shared, plain):
            b.close()
