"""The point-record ingest on the GPU (csrc/record_ingest.hip: rec_count_kernel, rec_scatter_kernel): locgpu_batch_upload_records[_deskew],
locgpu_cloud_upload_records[_deskew], locgpu_records_deskew_debug / _matrices and locgpu_records_ingest_times against the numpy
restatement (tests/record_ingest_ref.py, tests/range_deskew_ref.py) on the layouts, scans and point-time sets of
tests/record_ingest_cases.py.

As in test_gpu_range_deskew.py the check is split so that no coordinate needs a tolerance. (1) The matrices the device computed per
survivor are compared with the longdouble restatement; the bar is 8 units (the rule of tests/test_gpu_ndt_hb.py), a unit being the
float64 restatement's own worst deviation from the longdouble one on that track over all time sets (record_ingest_cases.unit, printed
by test_record_ingest_ref.py). (2) Given the matrices downloaded from the device, every point must equal range_deskew_ref.apply of the
raw restated point byte for byte, and counts and ring bytes must be the plain restatement's. (3) Records made of a range image's
survivors must leave the bytes locgpu_batch_upload_ranges_deskew leaves for the image.

Scans hold 0, 1, 63, 64, 65, 1023, 1024, 1025 and 4113 records: empty and partial tiles and the boundaries of every power-of-two
tile up to 4096 (the kernels' tile is 256 records).

Observed on an MI355X: the device's matrices deviate from the longdouble restatement by 0.92 (k2), 1.01 (k9_neg), 0.86 (k33_small),
1.16 (k5_equalq), 1.00 (k4_short) and 1.05 (k256) units, the same with F32 and with F64 time fields (1.8e-14 ... 2.4e-14 at
||t|| = 108 m; bars 1.3e-13 ... 1.8e-13). All points, counts and ring bytes equal; the whole file runs in about a second."""
import ctypes

import numpy as np
import pytest

import range_deskew_cases as dcases
import range_deskew_ref as dref
import record_ingest_cases as cases
import record_ingest_ref as rref

pytestmark = pytest.mark.gpu

INVALID = -1  # LOCGPU_ERR_INVALID
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0.0])
BATCH_SIZES = (1025, 0, 4096 + 17, 63, 1, 64, 1023, 65)  # eight scans; 1024 rides in the four-scan batches below
FOUR = (4096 + 17, 1024, 0, 1025)
TIMED = ("velodyne", "rslidar", "ouster", "velodyne_packed", "wide64")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scans():
    """The raw scans by size, computed once and never modified: (xyz, ring, intensity, dropped)."""
    return {n: cases.scan(n, 100 + n) for n in cases.SIZES}


def _blob(layout, scan, times=None, time_set="uniform", garbage=True):
    """(blob, time_offset, knot-clock origin) of one scan in one layout, its time field (if any) holding `time_set` of the track with
    knot times `times`, dropped records carrying garbage times."""
    xyz, ring, inten, dropped = scan
    L = rref.full(layout)
    tf, off, origin = None, 0.0, 0.0
    if L["time_kind"] != rref.TIME_NONE:
        rel, origin = cases.rel_times(times if times is not None else np.array([0.0, 0.1]), len(xyz), time_set)
        tf, off = cases.encode(L, rel, origin)
        if garbage:
            tf = cases.garbage_times(L, tf, dropped)
    return rref.pack(L, xyz, tf, ring, inten, seed=len(xyz)), off, origin


def _state(b, rings=True):
    return [(b.download_scan(s), b.download_rings(s) if rings else None) for s in range(b.n_local)]


# ---- 1. the plain form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.LAYOUTS))
def test_plain_form_equals_the_restatement_byte_for_byte(api, ctx, scans, name):
    layout = cases.LAYOUTS[name]
    arg = getattr(api, cases.READY[name]) if name in cases.READY else layout
    has_ring = rref.full(layout)["ring_kind"] != rref.RING_NONE
    for sizes in (BATCH_SIZES, FOUR):
        blobs = [_blob(layout, scans[n])[0] for n in sizes]
        want = [rref.survivors(layout, bl, n) for bl, n in zip(blobs, sizes)]
        b = ctx.batch_empty(len(sizes), max(sizes))
        cloud = api.Cloud(ctx)
        try:
            counts = b.upload_records(arg, blobs)
            assert counts.tolist() == [len(w[0]) for w in want]
            for s, (raw, rings, inten, _) in enumerate(want):
                pts = b.download_scan(s)
                assert _same(pts, raw) and not _bits(pts[:, 3]).any(), (name, s)
                if has_ring:
                    assert np.array_equal(b.download_rings(s), rings), (name, s)
                # the cloud form: the same x, y, z, the intensity in the fourth lane, dense
                got_rings = cloud.upload_records(arg, blobs[s])
                full = cloud.download()
                assert cloud.info == (len(raw), True)
                assert _same(full[:, :3], raw[:, :3]) and _same(full[:, 3], inten), (name, s)
                assert (got_rings is None and not has_ring) or np.array_equal(got_rings, rings)
            if not has_ring:
                with pytest.raises(api.LocGpuError) as err:
                    b.download_rings(0)
                assert "no resident rings" in str(err.value)
        finally:
            b.close()
            cloud.close()


def _deskew_case(layout, scan_list, track, time_sets, whichs):
    """Blobs, offsets and motion for one deskewed call: scan i on `track` with time set time_sets[i] and reference time whichs[i]."""
    times, poses = dcases.track(track)
    blobs, offs, kts, rts = [], [], [], []
    for sc, ts, which in zip(scan_list, time_sets, whichs):
        bl, off, origin = _blob(layout, sc, times, ts)
        blobs.append(bl)
        offs.append(off)
        kts.append(times + origin)
        rts.append(cases.ref_time(times + origin, which))
    return blobs, np.array(offs), np.array(kts), np.tile(poses, (len(blobs), 1, 1)), np.array(rts)


# ---- 2. the matrices against the longdouble restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["velodyne", "rslidar"])
@pytest.mark.parametrize("track", dcases.TRACKS)
def test_matrices_within_8_units_of_the_longdouble_restatement(ctx, scans, name, track):
    layout = cases.LAYOUTS[name]
    _, poses = dcases.track(track)
    unit, _ = cases.unit(track)
    bar = dcases.BAR_FACTOR * unit * dcases.scale(poses)
    n = 1025
    sets = cases.TIME_SETS
    whichs = [cases.REF_TIMES[i % 3] for i in range(len(sets))]
    blobs, offs, kt, kp, rt = _deskew_case(layout, [scans[n]] * len(sets), track, sets, whichs)
    b = ctx.batch_empty(len(sets), n)
    worst = 0.0
    try:
        ctx.records_deskew_debug(True)
        b.upload_records_deskew(layout, blobs, offs, kt, kp, rt)
        for s in range(len(sets)):
            tp = rref.survivors(layout, blobs[s], n, offs[s])[3]
            got = ctx.records_deskew_matrices(s)
            want = dref.matrices(kt[s], kp[s], tp, rt[s], np.longdouble)
            assert got.shape == (len(tp), 3, 4) and len(tp) > 500 and np.isfinite(got).all()
            worst = max(worst, float(np.abs(got.astype(np.longdouble) - want).max()))
    finally:
        ctx.records_deskew_debug(False)
        b.close()
    print("%s %s: worst |M - M_longdouble| %.3e = %.2f units (unit %.3f x %.3e, bar %.3e)"
          % (track, name, worst, worst / (unit * dcases.scale(poses)), unit, dcases.scale(poses), bar))
    assert worst <= bar, (track, name)


# ---- 3. the points, byte for byte, given the device's matrices -------------------------------------------------------------------------
@pytest.mark.parametrize("name", TIMED)
@pytest.mark.parametrize("track", dcases.TRACKS)
def test_points_equal_the_restatement_byte_for_byte(ctx, scans, name, track):
    layout = cases.LAYOUTS[name]
    k = dcases.TRACKS.index(track) + TIMED.index(name)
    sets = [cases.TIME_SETS[(k + i) % len(cases.TIME_SETS)] for i in range(4)]  # every set on every layout and track over the matrix
    blobs, offs, kt, kp, rt = _deskew_case(layout, [scans[n] for n in FOUR], track, sets, ("last", "first_knot", "mid", "last"))
    b = ctx.batch_empty(4, max(FOUR))
    try:
        ctx.records_deskew_debug(True)
        counts = b.upload_records_deskew(layout, blobs, offs, kt, kp, rt)
        moved = 0.0
        for s, n in enumerate(FOUR):
            raw, rings, _, _ = rref.survivors(layout, blobs[s], n, offs[s])
            pts, mats = b.download_scan(s), ctx.records_deskew_matrices(s)
            assert counts[s] == len(raw) == len(pts) == len(mats), (s, counts[s], len(raw))
            assert np.array_equal(b.download_rings(s), rings), s
            assert _same(pts, dref.apply(raw, np.arange(len(raw)), mats)) and not _bits(pts[:, 3]).any(), s
            if len(raw):
                moved = max(moved, float(np.abs(pts[:, :3] - raw[:, :3]).max()))
        print(name, track, sets, counts.tolist(), "largest displacement %.3f m" % moved)
        assert moved > 0.05  # the tracks move the sensor by decimetres to metres: a kernel that ignored them would pass nothing above
    finally:
        ctx.records_deskew_debug(False)
        b.close()


# ---- 4. equal to the range-image path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sensor", [("A", 4, 300), ("C", 5, 1231)])
def test_records_of_a_range_image_leave_the_bytes_of_the_range_path(api, synth, ctx, sensor):
    import test_gpu_range_deskew as rd  # sensors A and C and the image `holes` are that file's
    _, n_rings, n_cols = sensor
    model = api.SensorModel(n_rings, n_cols, rd.SCALE, rd.MIN_RANGE, *rd._tables(synth, n_rings, n_cols, False))
    holes = rd._images(model.cells, 11 + n_rings)[2]
    raw, rings, cols = dref.survivors(model, holes)  # ring-then-column order
    times, poses = dcases.track("k9_neg")
    col = dcases.col_times(times, n_cols, "rolled")
    whichs = ("last_col", "first_knot", "mid")
    rt = np.array([dcases.ref_time(times, col, w) for w in whichs])
    kt, kp = np.tile(times, (3, 1)), np.tile(poses, (3, 1, 1))
    layout = dict(stride_bytes=24, xyz_offset=0, time_offset=12, time_kind=rref.TIME_F64, ring_offset=20, ring_kind=rref.RING_U8)
    blob = rref.pack(layout, raw[:, :3], col[cols], rings)
    sn = api.Sensor(ctx, model)
    a, b = ctx.batch_empty(3, model.cells), ctx.batch_empty(3, model.cells)
    try:
        sn.set_col_times(col)
        c0 = a.upload_ranges_deskew(sn, [holes] * 3, kt, kp, rt)
        c1 = b.upload_records_deskew(layout, [blob] * 3, np.zeros(3), kt, kp, rt)
        assert c0.tolist() == c1.tolist() == [len(raw)] * 3 and len(raw) > 0
        for (p0, r0), (p1, r1) in zip(_state(a), _state(b)):
            assert _same(p0, p1) and np.array_equal(r0, r1)
    finally:
        a.close()
        b.close()
        sn.close()


# ---- 5. the identity track leaves the plain call's bytes --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["velodyne_packed", "ouster"])
def test_identity_track_leaves_the_bytes_of_the_plain_call(ctx, scans, name):
    layout = cases.LAYOUTS[name]
    for K in (2, 7):
        times = np.linspace(0.0, 0.1, K)
        blobs = [_blob(layout, scans[n], times, ts)[0] for n, ts in zip(FOUR, ("on_knots", "late", "uniform", "shuffled"))]
        plain, desk = ctx.batch_empty(4, max(FOUR)), ctx.batch_empty(4, max(FOUR))
        try:
            c0 = plain.upload_records(layout, blobs)
            c1 = desk.upload_records_deskew(layout, blobs, np.zeros(4), np.tile(times, (4, 1)), np.tile(IDENTITY, (4, K, 1)), [0.1, 0.0, 0.033, 0.3])
            assert c0.tolist() == c1.tolist() and c0[0] > 2000
            for (p0, r0), (p1, r1) in zip(_state(plain), _state(desk)):
                assert _same(p0, p1) and np.array_equal(r0, r1)
        finally:
            plain.close()
            desk.close()


# ---- 6. batch independence, the cloud form ----------------------------------------------------------------------------------------------
def test_a_scan_does_not_depend_on_its_batch_and_the_cloud_form_equals_it(api, ctx, scans):
    layout = cases.LAYOUTS["velodyne"]
    n = 4096 + 17
    t_a, p_a = dcases.track("k9_neg")
    p_b = p_a.copy()
    p_b[:, 4:] += np.linspace(0.0, 3.0, len(t_a))[:, None]  # another motion for the other scans of the batch
    mine, off, _ = _blob(layout, scans[n], t_a, "shuffled")
    other = _blob(layout, scans[1025], t_a, "uniform")[0]
    r_a, r_b = cases.ref_time(t_a, "mid"), cases.ref_time(t_a, "last")

    def run(place, count, debug=True):
        kp, rt = np.tile(p_b, (count, 1, 1)), np.full(count, r_b)
        kp[place], rt[place] = p_a, r_a
        blobs = [other] * count
        blobs[place] = mine
        b = ctx.batch_empty(count, n)
        try:
            ctx.records_deskew_debug(debug)
            b.upload_records_deskew(layout, blobs, np.full(count, off), np.tile(t_a, (count, 1)), kp, rt)
            return b.download_scan(place), b.download_rings(place), ctx.records_deskew_matrices(place) if debug else None
        finally:
            ctx.records_deskew_debug(False)
            b.close()

    alone = run(0, 1)
    assert len(alone[0]) == len(rref.survivors(layout, mine, n)[0]) > 2000 and len(alone[2]) == len(alone[0])
    for place, count in ((0, 4), (3, 4), (0, 1)):  # first and last of four, and a second run alone
        got = run(place, count)
        assert _same(got[0], alone[0]) and np.array_equal(got[1], alone[1]) and _same(got[2], alone[2]), (place, count)
    quiet = run(2, 4, debug=False)  # with the debug switch off: the same points, and no matrices are kept
    assert _same(quiet[0], alone[0]) and np.array_equal(quiet[1], alone[1])
    with pytest.raises(api.LocGpuError):
        ctx.records_deskew_matrices(0)
    cloud = api.Cloud(ctx)
    try:
        ctx.records_deskew_debug(True)
        rings = cloud.upload_records_deskew(layout, mine, off, t_a, p_a, r_a)
        full = cloud.download()
        assert cloud.info == (len(alone[0]), True)
        assert _same(full[:, :3], alone[0][:, :3]) and _same(full[:, 3], rref.survivors(layout, mine, n)[2]) and np.array_equal(rings, alone[1])
        assert _same(ctx.records_deskew_matrices(0), alone[2])
        assert cloud.upload_records_deskew(layout, b"", off, t_a, p_a, r_a, with_rings=False) is None and len(cloud) == 0
    finally:
        ctx.records_deskew_debug(False)
        cloud.close()


# ---- 7. refusals leave the target as it was ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_and_the_cloud_as_they_were(api, ctx, scans):
    L = api.lib()
    layout = cases.LAYOUTS["rslidar"]
    times, poses = dcases.track("k9_neg")
    sizes = (1025, 65, 1023, 1024)
    made = [_blob(layout, scans[n], times, "uniform") for n in sizes]
    blobs = [m[0] for m in made]
    want_counts = [len(rref.survivors(layout, bl, n)[0]) for bl, n in zip(blobs, sizes)]
    good = (np.zeros(4), np.tile(times, (4, 1)), np.tile(poses, (4, 1, 1)), np.full(4, times[-1]))

    def refused(call):
        with pytest.raises(api.LocGpuError) as err:
            call()
        assert err.value.code == INVALID and len(str(err.value)) > 20
        return err.value

    def with_time(n, survivor_index, value):
        """scan of size n with the time of its survivor number `survivor_index` replaced."""
        xyz, ring, inten, dropped = scans[n]
        rel, origin = cases.rel_times(times, n, "uniform")
        tf = cases.garbage_times(layout, cases.encode(layout, rel, origin)[0], dropped)
        tf[np.nonzero(~dropped)[0][survivor_index]] = value
        return rref.pack(layout, xyz, tf, ring, inten, seed=n)

    b = ctx.batch_empty(4, 1025)
    cloud = api.Cloud(ctx)
    try:
        b.upload_records_deskew(layout, blobs, *good)
        cloud.upload_records(layout, blobs[0])
        before, cloud_before = _state(b), cloud.download()
        assert [len(p) for p, _ in before] == want_counts

        def unchanged():
            after = _state(b)
            assert all(_same(p0, p1) and np.array_equal(r0, r1) for (p0, r0), (p1, r1) in zip(before, after))
            assert _same(cloud.download(), cloud_before) and cloud.info == (len(cloud_before), True)

        # a survivor time before the first knot, in scan 1 (two of them) and scan 2 (one): the first such scan is named
        early = list(blobs)
        early[1] = rref.pack(layout, *_two_bad(scans[65], layout, times, times[0] - 1e-6))
        early[2] = with_time(1023, 700, times[0] - 1.0)
        e = refused(lambda: b.upload_records_deskew(layout, early, *good))
        assert "scan 1 has 2 survivors" in str(e) and "unchanged" in str(e) and e.status.tolist() == [0, 1, 1, 0] and e.counts.tolist() == want_counts
        e = refused(lambda: cloud.upload_records_deskew(layout, early[2], 0.0, times, poses, times[-1]))
        assert "scan 0 has 1 survivors" in str(e)
        unchanged()
        # one 0.5001 s behind the last knot (0.2 s behind is served: the late time set)
        late = list(blobs)
        late[0] = with_time(1025, -1, times[-1] + 0.5001)
        e = refused(lambda: b.upload_records_deskew(layout, late, *good))
        assert "scan 0 has 1 survivors" in str(e) and "0.5 s" in str(e) and e.status.tolist() == [1, 0, 0, 0]
        refused(lambda: cloud.upload_records_deskew(layout, late[0], 0.0, times, poses, times[-1]))
        unchanged()
        # a NaN survivor time in the last scan only
        nan = list(blobs)
        nan[3] = with_time(1024, 500, np.nan)
        e = refused(lambda: b.upload_records_deskew(layout, nan, *good))
        assert "scan 3" in str(e) and e.status.tolist() == [0, 0, 0, 1]
        unchanged()
        # capacity one short: the counts come back, the batch stays
        small = ctx.batch_empty(4, max(want_counts) - 1)
        try:
            few = [bl[:32 * 40] for bl in blobs]
            small.upload_records_deskew(layout, few, *good)
            keep_small = _state(small)
            for call in (lambda: small.upload_records_deskew(layout, blobs, *good), lambda: small.upload_records(layout, blobs)):
                e = refused(call)
                assert str(max(want_counts)) in str(e) and e.counts.tolist() == want_counts
                assert all(_same(p0, p1) and np.array_equal(r0, r1) for (p0, r0), (p1, r1) in zip(keep_small, _state(small)))
        finally:
            small.close()
        # a NULL records[1]; n_points out of range; a time offset that is not finite; TIME_NONE with deskew; the motion's refusals
        Lc = api.point_layout(layout)
        keep = [np.frombuffer(bytes(bl), np.uint8) for bl in blobs]
        ptrs = (ctypes.c_void_p * 4)(keep[0].ctypes.data, None, keep[2].ctypes.data, keep[3].ctypes.data)
        cnt = np.array(sizes, np.int64)
        m, keep_m = api.sweep_motion(4, *good[1:])
        offs = np.zeros(4)
        assert L.locgpu_batch_upload_records_deskew(b._h, ctypes.byref(Lc), ptrs, cnt.ctypes.data, offs.ctypes.data, ctypes.byref(m), None, None) == INVALID
        assert b"records[1]" in L.locgpu_last_error(ctx._h)
        assert L.locgpu_batch_upload_records(b._h, ctypes.byref(Lc), ptrs, cnt.ctypes.data, None) == INVALID and b"records[1]" in L.locgpu_last_error(ctx._h)
        ptrs[1] = keep[1].ctypes.data
        for bad_n in (-1, 16 * 1025 + 1):
            cnt2 = cnt.copy()
            cnt2[2] = bad_n
            assert L.locgpu_batch_upload_records(b._h, ctypes.byref(Lc), ptrs, cnt2.ctypes.data, None) == INVALID and b"n_points[2]" in L.locgpu_last_error(ctx._h)
        assert L.locgpu_batch_upload_records(b._h, ctypes.byref(Lc), None, cnt.ctypes.data, None) == INVALID
        offs[2] = np.inf
        assert L.locgpu_batch_upload_records_deskew(b._h, ctypes.byref(Lc), ptrs, cnt.ctypes.data, offs.ctypes.data, ctypes.byref(m), None, None) == INVALID
        assert b"time_offsets[2]" in L.locgpu_last_error(ctx._h)
        assert "LOCGPU_TIME_NONE" in str(refused(lambda: b.upload_records_deskew(dict(layout, time_kind=rref.TIME_NONE), blobs, *good)))
        assert "n_knots" in str(refused(lambda: b.upload_records_deskew(layout, blobs, np.zeros(4), np.zeros((4, 1)), np.tile(IDENTITY, (4, 1, 1)), np.zeros(4))))
        kt = good[1].copy()
        kt[3, 3] = kt[3, 2]
        e = refused(lambda: b.upload_records_deskew(layout, blobs, good[0], kt, good[2], good[3]))
        assert "increasing" in str(e) and "scan 3" in str(e)
        assert "0.5 s" in str(refused(lambda: b.upload_records_deskew(layout, blobs, good[0], good[1], good[2], np.full(4, times[-1] + 0.6))))
        assert "before the first knot" in str(refused(lambda: cloud.upload_records_deskew(layout, blobs[0], 0.0, times, poses, times[0] - 1e-3)))
        assert L.locgpu_batch_upload_records_deskew(b._h, ctypes.byref(Lc), ptrs, cnt.ctypes.data, np.zeros(4).ctypes.data, None, None, None) == INVALID
        assert b"motion" in L.locgpu_last_error(ctx._h)
        unchanged()
        # an alignment begun and not ended
        ctx.icp_set_target(before[0][0][:, :3])
        ctx.icp_align_batch_begin(b, np.tile(IDENTITY, (4, 1)), api.icp_opts(method=api.P2P, max_iteration=2))
        try:
            assert "begun" in str(refused(lambda: b.upload_records_deskew(layout, blobs, *good)))
            assert "begun" in str(refused(lambda: b.upload_records(layout, blobs)))
        finally:
            ctx.align_batch_end(b)
        unchanged()
        # and after all of them the call still works
        assert b.upload_records_deskew(layout, blobs, *good).tolist() == want_counts
        assert all(_same(p0, p1) and np.array_equal(r0, r1) for (p0, r0), (p1, r1) in zip(before, _state(b)))
    finally:
        b.close()
        cloud.close()


def _two_bad(scan, layout, times, value):
    """pack()'s arguments for `scan` with the times of its survivors 3 and 20 replaced by `value`."""
    xyz, ring, inten, dropped = scan
    rel, origin = cases.rel_times(times, len(xyz), "uniform")
    tf = cases.garbage_times(layout, cases.encode(layout, rel, origin)[0], dropped)
    kept = np.nonzero(~dropped)[0]
    tf[kept[3]] = tf[kept[20]] = value
    return xyz, tf, ring, inten


# ---- 8. downstream ----------------------------------------------------------------------------------------------------------------------
def test_loam_picker_and_alignment_downstream(api, synth, ctx):
    n_rings, n_cols = 4, 300
    model = api.SensorModel(n_rings, n_cols, 0.002, 4.0, *synth.sensor_tables(n_rings, n_cols))
    image = synth.make_range_image(3, model).reshape(-1)
    raw_pts, rings, cols = dref.survivors(model, image)
    times, poses = dcases.track("k33_small")  # 1.5 m and 3.2 mrad over the sweep: rings stay rings
    col = dcases.col_times(times, n_cols, "uniform")
    layout = cases.LAYOUTS["velodyne"]
    blob = rref.pack(layout, raw_pts[:, :3], col[cols].astype(np.float32), rings, np.arange(len(rings)) % 200)
    raw, host = ctx.batch_empty(4, 1200), ctx.batch_empty(4, 1200)
    edge, surf = ctx.batch_empty(4, 4 * 6 * 20), ctx.batch_empty(4, 1200)
    flt = ctx.batch_empty(4, 1200)
    try:
        rt = [cases.ref_time(times, w) for w in ("last", "mid", "first_knot", "mid")]
        raw.upload_records_deskew(layout, [blob, blob[:32 * 500], blob[:32 * 777], blob], np.zeros(4), np.tile(times, (4, 1)), np.tile(poses, (4, 1, 1)), rt)
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
        counts, status = raw.preprocess(0.5, out=flt)
        assert counts[0] > 0 and counts[1] > 0
        ctx.icp_set_target(synth.make_local_map(2000, 3, half=40.0))
        out_poses, stats = ctx.icp_align_batch(flt, np.array([synth.make_pose(3)[1]] * 4), api.icp_opts(method=api.P2P, max_iteration=5))
        assert np.isfinite(out_poses).all() and len(stats) == 4 and any(s["iterations"] >= 1 for s in stats)
    finally:
        for b in (raw, host, edge, surf, flt):
            b.close()


# ---- 9. profiling; the range paths' times are their own ------------------------------------------------------------------------------------
def test_times_are_reported_and_the_range_times_are_left_alone(api, ctx, scans):
    layout = cases.LAYOUTS["ouster"]
    times, poses = dcases.track("k2")
    blobs = [_blob(layout, scans[n], times, "ns")[0] for n in FOUR]
    b = ctx.batch_empty(4, max(FOUR))
    try:
        range_before = (ctx.range_ingest_times(), ctx.range_deskew_times())
        ctx.profile_enable(True)
        b.upload_records(layout, blobs)
        plain = ctx.records_ingest_times()
        assert 0 < plain[0] < 1e3 and 0 < plain[1] < 1e3
        b.upload_records_deskew(layout, blobs, np.zeros(4), np.tile(times, (4, 1)), np.tile(poses, (4, 1, 1)), np.full(4, times[-1]))
        desk = ctx.records_ingest_times()
        print("record ingest times: plain copies %.3f ms, kernels %.3f ms; deskewed copies %.3f ms, kernels %.3f ms" % (*plain, *desk))
        assert 0 < desk[0] < 1e3 and 0 < desk[1] < 1e3 and desk != plain
        assert (ctx.range_ingest_times(), ctx.range_deskew_times()) == range_before
    finally:
        ctx.profile_enable(False)
        b.close()
