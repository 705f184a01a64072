"""The motion-compensated range-image ingest on the GPU (csrc/range_ingest.hip: rd_pose_kernel, rd_scatter_kernel):
locgpu_sensor_set_col_times, locgpu_batch_upload_ranges_deskew, locgpu_cloud_upload_ranges_deskew, locgpu_range_deskew_matrices and
locgpu_range_deskew_times against the numpy restatement (tests/range_deskew_ref.py) on the tracks, column-time tables and reference
times of tests/range_deskew_cases.py.

The check is split so that no coordinate needs a tolerance. (1) The matrices the device computed are compared with the longdouble
restatement: the bar is 8 units (the rule of tests/test_gpu_ndt_hb.py), a unit being the float64 restatement's own worst deviation
from the longdouble one on that track — measured by range_deskew_cases.unit at run time and printed by
test_range_deskew_ref.py::test_unit_of_the_float64_restatement, in multiples of eps * max(1, max ||t||), eps = 2^-52, ||t|| = 108 m:

    track      unit (300 columns)  unit (1231 columns)   →  bar at 300 columns
    k2         0.931               1.005                     1.81e-13
    k9_neg     0.898               1.397                     1.73e-13
    k33_small  0.839               0.973                     1.63e-13
    k5_equalq  0.699               1.031                     1.34e-13
    k4_short   0.949               1.047                     1.84e-13
    k256       0.905               0.823                     1.76e-13

(2) Given the matrices downloaded from the device, every point must equal range_deskew_ref.apply of the raw restated point byte for
byte, and counts and ring bytes must be the plain restatement's.

The sensors are those of tests/test_gpu_range_ingest.py, rebuilt here. A: 4 rings x 300 columns (one tile). B: 16 x 64 with per-laser
azimuth tables. C: 5 x 1231 = 6155 cells (four tiles, the last partial, a last 16-byte load of three cells). D: 256 x 2100 (263 tiles,
ring bytes up to 255, nine trips of rd_pose_kernel's column loop). Four images per sensor: all zero; all hit; about 30 % holes with
near returns mixed in; every return below min_range.

Observed on an MI355X: the device's matrices deviate from the longdouble restatement by 1.00 unit on every track and both sensors
(k2 2.26e-14 / 2.44e-14, k9_neg 2.17e-14 / 3.37e-14, k33_small 2.03e-14 / 2.36e-14, k5_equalq 1.67e-14 / 2.47e-14, k4_short 2.30e-14 /
2.54e-14, k256 2.20e-14 / 2.00e-14 at 300 / 1231 columns) — exactly the float64 restatement's own deviation: the device library's acos
and sin change nothing at this scale. All points, counts and ring bytes equal."""
import ctypes

import numpy as np
import pytest

import range_deskew_cases as cases
import range_deskew_ref as dref

pytestmark = pytest.mark.gpu

INVALID = -1  # LOCGPU_ERR_INVALID
SCALE, MIN_RANGE = 0.002, 4.0
LEAF = 0.5
SENSORS = (("A", 4, 300, False), ("B", 16, 64, True), ("C", 5, 1231, False), ("D", 256, 2100, False))
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0.0])


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
    """Per sensor: the model, its resident form, four images and the restatement's (raw points, rings, columns) of each. Computed once,
    never modified."""
    w = {}
    for name, n_rings, n_cols, per_ring in SENSORS:
        model = api.SensorModel(n_rings, n_cols, SCALE, MIN_RANGE, *_tables(synth, n_rings, n_cols, per_ring))
        images = _images(model.cells, 11 + n_rings)
        want = [dref.survivors(model, im) for im in images]
        assert len(want[0][0]) == 0 and len(want[1][0]) == model.cells and 0 < len(want[2][0]) < 0.75 * model.cells and len(want[3][0]) == 0
        w[name] = dict(model=model, sensor=api.Sensor(ctx, model), images=images, want=want)
    yield w
    for v in w.values():
        v["sensor"].close()


def _state(b):
    """Everything a batch with resident rings holds, as downloaded."""
    return [(b.download_scan(s), b.download_rings(s)) for s in range(b.n_local)]


def _motion(track, col, whichs):
    """One scan per reference time of `whichs`, all on `track`: (knot_times [n, K], knot_poses [n, K, 7], ref_times [n])."""
    times, poses = cases.track(track)
    n = len(whichs)
    return np.tile(times, (n, 1)), np.tile(poses, (n, 1, 1)), np.array([cases.ref_time(times, col, w) for w in whichs])


# ---- 1. the matrices against the longdouble restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("track", cases.TRACKS)
def test_matrices_within_8_units_of_the_longdouble_restatement(ctx, world, track):
    times, poses = cases.track(track)
    for name in ("A", "C"):
        v = world[name]
        n_cols = v["model"].n_cols
        unit = cases.unit(track, n_cols)
        bar = cases.BAR_FACTOR * unit * cases.scale(poses)
        worst = 0.0
        b = ctx.batch_empty(len(cases.REF_TIMES), v["model"].cells)
        try:
            for table in cases.COL_TABLES:
                col = cases.col_times(times, n_cols, table)
                v["sensor"].set_col_times(col)
                kt, kp, rt = _motion(track, col, cases.REF_TIMES)
                b.upload_ranges_deskew(v["sensor"], [v["images"][2]] * len(rt), kt, kp, rt)
                for s, r in enumerate(rt):
                    got = ctx.range_deskew_matrices(s)
                    want = dref.matrices(times, poses, col, r, np.longdouble)
                    assert got.shape == (n_cols, 3, 4) and np.isfinite(got).all()
                    worst = max(worst, float(np.abs(got.astype(np.longdouble) - want).max()))
        finally:
            b.close()
        print("%s sensor %s: worst |M - M_longdouble| %.3e = %.2f units (unit %.3f x %.3e, bar %.3e)"
              % (track, name, worst, worst / (unit * cases.scale(poses)), unit, cases.scale(poses), bar))
        assert worst <= bar, (track, name)


# ---- 2. the points, byte for byte, given the device's matrices -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in SENSORS])
@pytest.mark.parametrize("track", cases.TRACKS)
def test_points_equal_the_restatement_byte_for_byte(ctx, world, name, track):
    v = world[name]
    model, want = v["model"], v["want"]
    times, _ = cases.track(track)
    table = cases.COL_TABLES[(cases.TRACKS.index(track) + "ABCD".index(name)) % len(cases.COL_TABLES)]  # every table on every sensor and track over the matrix
    col = cases.col_times(times, model.n_cols, table)
    v["sensor"].set_col_times(col)
    whichs = ("last_col", "first_knot", "mid", "last_col")  # scan s shows image s
    kt, kp, rt = _motion(track, col, whichs)
    b = ctx.batch_empty(4, model.cells)
    try:
        counts = b.upload_ranges_deskew(v["sensor"], v["images"], kt, kp, rt)
        moved = 0.0
        for s in range(4):
            raw, rings, cols = want[s]
            pts, got_rings = b.download_scan(s), b.download_rings(s)
            mats = ctx.range_deskew_matrices(s)
            assert counts[s] == len(raw) == len(pts), (s, counts[s], len(raw))
            assert got_rings.dtype == np.uint8 and np.array_equal(got_rings, rings), s
            assert _same(pts, dref.apply(raw, cols, mats)) and not _bits(pts[:, 3]).any(), s
            if len(raw):
                moved = max(moved, float(np.abs(pts[:, :3] - raw[:, :3]).max()))
        print(name, track, table, counts.tolist(), "largest displacement %.3f m" % moved)
        assert moved > 0.05  # the tracks move the sensor by decimetres to metres: a decode that ignored them would pass nothing above
    finally:
        b.close()


# ---- 3. the identity track leaves the plain call's bytes -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_identity_track_leaves_the_bytes_of_the_plain_call(ctx, world, name):
    v = world[name]
    cells = v["model"].cells
    for K in (2, 7):
        times = np.linspace(0.0, 0.1, K)
        v["sensor"].set_col_times(cases.col_times(times, v["model"].n_cols, "on_knots"))
        plain, desk = ctx.batch_empty(4, cells), ctx.batch_empty(4, cells)
        try:
            c0 = plain.upload_ranges(v["sensor"], v["images"])
            c1 = desk.upload_ranges_deskew(v["sensor"], v["images"], np.tile(times, (4, 1)), np.tile(IDENTITY, (4, K, 1)), [0.1, 0.0, 0.033, 0.3])
            assert c0.tolist() == c1.tolist()
            for (p0, r0), (p1, r1) in zip(_state(plain), _state(desk)):
                assert _same(p0, p1) and np.array_equal(r0, r1)
        finally:
            plain.close()
            desk.close()


# ---- 4. batch independence, the cloud form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_a_scan_does_not_depend_on_its_batch_and_the_cloud_form_equals_it(api, ctx, world, name):
    v = world[name]
    cells, sensor, images = v["model"].cells, v["sensor"], v["images"]
    t_a, p_a = cases.track("k9_neg")
    t_b, p_b = cases.track("k9_neg")
    p_b = p_b.copy()
    p_b[:, 4:] += np.linspace(0.0, 3.0, len(t_b))[:, None]  # another motion for the other scans of the batch
    col = cases.col_times(t_a, v["model"].n_cols, "rolled")
    sensor.set_col_times(col)
    r_a, r_b = cases.ref_time(t_a, col, "mid"), cases.ref_time(t_b, col, "last_col")

    def run(place, n):
        kt, kp, rt = np.tile(t_b, (n, 1)), np.tile(p_b, (n, 1, 1)), np.full(n, r_b)
        kt[place], kp[place], rt[place] = t_a, p_a, r_a
        ims = [images[1]] * n
        ims[place] = images[2]
        b = ctx.batch_empty(n, cells)
        try:
            b.upload_ranges_deskew(sensor, ims, kt, kp, rt)
            return b.download_scan(place), b.download_rings(place), ctx.range_deskew_matrices(place)
        finally:
            b.close()

    alone = run(0, 1)
    assert len(alone[0]) == len(v["want"][2][0]) > 0
    for place, n in ((0, 4), (3, 4), (0, 1)):  # first and last of four, and a second run alone
        got = run(place, n)
        assert _same(got[0], alone[0]) and np.array_equal(got[1], alone[1]) and _same(got[2], alone[2]), (place, n)
    cloud = api.Cloud(ctx)
    try:
        rings = cloud.upload_ranges_deskew(sensor, images[2], t_a, p_a, r_a)
        assert cloud.info == (len(alone[0]), True)
        assert _same(cloud.download(), alone[0]) and np.array_equal(rings, alone[1])
        assert _same(ctx.range_deskew_matrices(0), alone[2])
        assert cloud.upload_ranges_deskew(sensor, images[0], t_a, p_a, r_a, with_rings=False) is None and len(cloud) == 0
    finally:
        cloud.close()


# ---- 5. refusals leave the target as it was ------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_and_the_cloud_as_they_were(api, synth, ctx, world):
    L = api.lib()
    v = world["A"]
    model, images = v["model"], v["images"]
    sensor = api.Sensor(ctx, model)  # a sensor of its own: it starts without column times
    times, poses = cases.track("k9_neg")
    K = len(times)
    col = cases.col_times(times, model.n_cols, "uniform")
    good = (np.tile(times, (4, 1)), np.tile(poses, (4, 1, 1)), np.full(4, col[-1]))

    def refused(call):
        with pytest.raises(api.LocGpuError) as err:
            call()
        assert err.value.code == INVALID and len(str(err.value)) > 20
        return err.value

    b = ctx.batch_empty(4, model.cells)
    cloud = api.Cloud(ctx)
    try:
        fresh = api.Context(0)  # no deskewed call has run on it
        try:
            assert "no deskewed ingest" in str(refused(lambda: fresh.range_deskew_matrices(0)))
            assert fresh.range_deskew_times() == (0.0, 0.0, 0.0)
        finally:
            fresh.close()
        refused(lambda: ctx.range_deskew_matrices(99))
        b.upload_ranges(sensor, images)
        cloud.upload_ranges(sensor, images[2])
        before, cloud_before = _state(b), cloud.download()

        def unchanged():
            after = _state(b)
            assert all(_same(p0, p1) and np.array_equal(r0, r1) for (p0, r0), (p1, r1) in zip(before, after))
            assert _same(cloud.download(), cloud_before)

        # a sensor without column times
        assert "column times" in str(refused(lambda: b.upload_ranges_deskew(sensor, images, *good)))
        refused(lambda: cloud.upload_ranges_deskew(sensor, images[2], times, poses, col[-1]))
        unchanged()
        bad = col.copy()
        bad[5] = np.inf
        refused(lambda: sensor.set_col_times(bad))
        assert L.locgpu_sensor_set_col_times(sensor._h, None) == INVALID
        sensor.set_col_times(col)

        def both(kt, kp, rt, word):
            e = refused(lambda: b.upload_ranges_deskew(sensor, images, kt, kp, rt))
            assert word in str(e), (word, str(e))
            e = refused(lambda: cloud.upload_ranges_deskew(sensor, images[2], kt[0], kp[0], rt[0]))
            assert word in str(e), (word, str(e))
            unchanged()

        # a reference time 0.6 s behind the last knot; one before the first knot
        both(good[0], good[1], np.full(4, times[-1] + 0.6), "0.5 s")
        both(good[0], good[1], np.full(4, times[0] - 1e-3), "before the first knot")
        # K = 1 and K = 257
        both(np.zeros((4, 1)), np.tile(IDENTITY, (4, 1, 1)), np.zeros(4), "n_knots")
        both(np.tile(np.linspace(0.0, 0.1, 257), (4, 1)), np.tile(IDENTITY, (4, 257, 1)), np.full(4, 0.05), "n_knots")
        # knot times not increasing: equal neighbours, and a NaN
        kt = good[0].copy()
        kt[:, 3] = kt[:, 2]
        both(kt, good[1], good[2], "increasing")
        kt[:, 3] = np.nan
        both(kt, good[1], good[2], "increasing")
        # a fault in the LAST scan only is found too
        kt = good[0].copy()
        kt[3, 0] = col.min() + 1e-4
        e = refused(lambda: b.upload_ranges_deskew(sensor, images, kt, good[1], good[2]))
        assert "scan 3" in str(e)
        unchanged()
        # a column time before the first knot; one more than 0.5 s behind the last
        early = col.copy()
        early[17] = times[0] - 1e-6
        sensor.set_col_times(early)
        both(*good, "before the first knot")
        late = col.copy()
        late[200] = times[-1] + 0.5001
        sensor.set_col_times(late)
        both(*good, "0.5 s")
        sensor.set_col_times(col)
        # a NULL motion and a NULL array inside it
        ptrs = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in images])
        m, keep = api.sweep_motion(4, *good)
        assert L.locgpu_batch_upload_ranges_deskew(b._h, sensor._h, ptrs, None, None) == INVALID and b"motion" in L.locgpu_last_error(ctx._h)
        for field in ("knot_times", "knot_poses", "ref_times"):
            m2, keep2 = api.sweep_motion(4, *good)
            setattr(m2, field, None)
            assert L.locgpu_batch_upload_ranges_deskew(b._h, sensor._h, ptrs, ctypes.byref(m2), None) == INVALID and b"NULL" in L.locgpu_last_error(ctx._h)
            assert L.locgpu_cloud_upload_ranges_deskew(cloud._h, sensor._h, images[2].ctypes.data, ctypes.byref(m2), None, None) == INVALID
        # the plain call's refusals: a NULL image, a NULL sensor
        ptrs_bad = (ctypes.c_void_p * 4)(images[0].ctypes.data, None, images[2].ctypes.data, images[3].ctypes.data)
        assert L.locgpu_batch_upload_ranges_deskew(b._h, sensor._h, ptrs_bad, ctypes.byref(m), None) == INVALID and b"images[1]" in L.locgpu_last_error(ctx._h)
        assert L.locgpu_batch_upload_ranges_deskew(b._h, None, ptrs, ctypes.byref(m), None) == INVALID
        unchanged()
        # capacity too small: the counts come back, the batch stays
        small = ctx.batch_empty(4, model.cells - 1)
        try:
            few = [im.copy() for im in images]
            for a in few:
                a[100:] = 0
            small.upload_ranges_deskew(sensor, few, *good)
            keep_small = _state(small)
            e = refused(lambda: small.upload_ranges_deskew(sensor, images, *good))
            assert str(model.cells) in str(e) and e.counts.tolist() == [len(w[0]) for w in v["want"]]
            assert all(_same(p0, p1) and np.array_equal(r0, r1) for (p0, r0), (p1, r1) in zip(keep_small, _state(small)))
        finally:
            small.close()
        # an alignment begun and not ended
        ctx.icp_set_target(v["want"][1][0][:, :3])
        ctx.icp_align_batch_begin(b, np.tile(IDENTITY, (4, 1)), api.icp_opts(method=api.P2P, max_iteration=2))
        try:
            assert "begun" in str(refused(lambda: b.upload_ranges_deskew(sensor, images, *good)))
        finally:
            ctx.align_batch_end(b)
        unchanged()
        # and after all of them the call still works
        counts = b.upload_ranges_deskew(sensor, images, *good)
        assert counts.tolist() == [len(w[0]) for w in v["want"]]
    finally:
        b.close()
        cloud.close()
        sensor.close()


# ---- 6. downstream -------------------------------------------------------------------------------------------------------------------
def test_loam_picker_and_alignment_downstream(api, synth, ctx, world):
    v = world["A"]
    model, sensor = v["model"], v["sensor"]
    scan = synth.make_range_image(3, model).reshape(-1)
    images = [scan, v["images"][1], v["images"][2], scan]
    times, poses = cases.track("k33_small")  # 1.5 m and 3.2 mrad over the sweep: rings stay rings
    col = cases.col_times(times, model.n_cols, "uniform")
    sensor.set_col_times(col)
    kt, kp, rt = _motion("k33_small", col, ("last_col", "mid", "first_knot", "mid"))
    raw, host = ctx.batch_empty(4, 1200), ctx.batch_empty(4, 1200)
    edge, surf = ctx.batch_empty(4, 4 * 6 * 20), ctx.batch_empty(4, 1200)
    flt = ctx.batch_empty(4, 1200)
    try:
        raw.upload_ranges_deskew(sensor, images, kt, kp, rt)
        got = _state(raw)
        ne, ns, st = raw.loam_extract_resident(4, edge, surf)
        res = [(edge.download_scan(s), surf.download_scan(s)) for s in range(4)]
        assert ne[0] > 0 and ns[0] > 0
        host.upload_async([p for p, _ in got])
        host.upload_wait()
        ne2, ns2, st2 = host.loam_extract([r for _, r in got], 4, edge, surf)
        assert ne.tolist() == ne2.tolist() and ns.tolist() == ns2.tolist() and st.tolist() == st2.tolist()
        for s in range(4):
            assert _same(edge.download_scan(s), res[s][0]) and _same(surf.download_scan(s), res[s][1]), s
        counts, status = raw.preprocess(LEAF, out=flt)
        assert counts[0] > 0 and counts[1] > 0
        ctx.icp_set_target(synth.make_local_map(2000, 3, half=40.0))
        out_poses, stats = ctx.icp_align_batch(flt, np.array([synth.make_pose(3)[1]] * 4), api.icp_opts(method=api.P2P, max_iteration=5))
        assert np.isfinite(out_poses).all() and len(stats) == 4 and any(s["iterations"] >= 1 for s in stats)
    finally:
        for b in (raw, host, edge, surf, flt):
            b.close()


# ---- 7 / 8. profiling; the plain call's times are its own ------------------------------------------------------------------------------
def test_deskew_times_are_reported_and_the_plain_times_stay_the_plain_calls(ctx, world):
    v = world["C"]
    times, _ = cases.track("k2")
    col = cases.col_times(times, v["model"].n_cols, "uniform")
    v["sensor"].set_col_times(col)
    kt, kp, rt = _motion("k2", col, ("last_col",) * 4)
    b = ctx.batch_empty(4, v["model"].cells)
    try:
        ctx.profile_enable(True)
        b.upload_ranges(v["sensor"], v["images"])
        plain = ctx.range_ingest_times()
        assert 0 < plain[0] < 1e3 and 0 < plain[1] < 1e3
        b.upload_ranges_deskew(v["sensor"], v["images"], kt, kp, rt)
        copy_ms, pose_ms, decode_ms = ctx.range_deskew_times()
        print("deskew times: copies %.3f ms, matrix kernel %.3f ms, decode kernels %.3f ms; plain %.3f / %.3f ms" % (copy_ms, pose_ms, decode_ms, *plain))
        assert 0 < copy_ms < 1e3 and 0 < pose_ms < 1e3 and 0 < decode_ms < 1e3
        assert ctx.range_ingest_times() == plain  # the deskewed call left them alone
        b.upload_ranges(v["sensor"], v["images"])
        assert ctx.range_deskew_times() == (copy_ms, pose_ms, decode_ms)
    finally:
        ctx.profile_enable(False)
        b.close()
