"""Deskew of a resident batch on the GPU (csrc/resident_deskew.hip: rsd_check_kernel, rsd_move_kernel; the kept-times variants of the
ingest scatter kernels): locgpu_batch_keep_times, locgpu_batch_download_times, locgpu_batch_deskew and locgpu_batch_deskew_times.

No coordinate needs a tolerance. Every comparison is byte for byte: the kept times against the numpy restatement's
(record_ingest_ref.survivors, the sensor's column table), the compensated points against the deskewed INGEST of the same scans,
offsets and motion (locgpu_batch_upload_records_deskew, locgpu_batch_upload_ranges_deskew), whose own chain to numpy is
test_gpu_record_ingest.py and test_gpu_range_deskew.py, and — so that the chain does not rest on the new code alone — against
range_deskew_ref.apply with the matrices the ingest form computed.

Scans hold 0 ... 4113 points: empty and partial tiles and both sides of the 64-, 256- and 1024-point edges (the ingest kernels' tile
is 256 records, the pass's 1024 points). The refusal for sharded batches is not exercised: it needs a communicator.

Observed on an MI355X: every comparison equal; the whole file runs in about a second."""
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
TIMED = ("velodyne", "rslidar", "ouster", "velodyne_packed")
SIX = (4096 + 17, 1024, 0, 1025, 1023, 65)  # one scan per time set of cases.TIME_SETS
REST = (1, 63, 64)                          # the sizes of cases.SIZES that SIX leaves out
WHICHS = ("last", "first_knot", "mid", "last", "mid", "first_knot")


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


def _blob(layout, scan, times, time_set):
    """(blob, time_offset, knot-clock origin) of one scan, its time field holding `time_set` of the track with knot times `times`,
    dropped records carrying garbage times."""
    xyz, ring, inten, dropped = scan
    rel, origin = cases.rel_times(times, len(xyz), time_set)
    tf, off = cases.encode(layout, rel, origin)
    return rref.pack(layout, xyz, cases.garbage_times(layout, tf, dropped), ring, inten, seed=len(xyz)), off, origin


def _case(layout, scan_list, track, time_sets, whichs):
    """Blobs, offsets and motion of one call: scan i on `track` with time set time_sets[i] and reference time whichs[i]."""
    times, poses = dcases.track(track)
    blobs, offs, kts, rts = [], [], [], []
    for sc, ts, which in zip(scan_list, time_sets, whichs):
        bl, off, origin = _blob(layout, sc, times, ts)
        blobs.append(bl)
        offs.append(off)
        kts.append(times + origin)
        rts.append(cases.ref_time(times + origin, which))
    return blobs, np.array(offs), dict(knot_times=np.array(kts), knot_poses=np.tile(poses, (len(blobs), 1, 1)), ref_times=np.array(rts))


def _remotion(track, origins, whichs):
    """The motion of another track on the clocks of an existing case."""
    times, poses = dcases.track(track)
    return dict(knot_times=np.array([times + o for o in origins]), knot_poses=np.tile(poses, (len(origins), 1, 1)),
                ref_times=np.array([cases.ref_time(times + o, w) for o, w in zip(origins, whichs)]))


def _state(b):
    return [(b.download_scan(s), b.download_rings(s)) for s in range(b.n_local)]


def _equal(a, b):
    return len(a) == len(b) and all(_same(p0, p1) and np.array_equal(r0, r1) for (p0, r0), (p1, r1) in zip(a, b))


def _refused(api, call):
    with pytest.raises(api.LocGpuError) as err:
        call()
    assert err.value.code == INVALID and len(str(err.value)) > 30
    return err.value


# ---- 1. the kept times -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TIMED)
def test_kept_times_equal_the_restatement_and_nothing_else_changes(api, ctx, scans, name):
    layout = cases.LAYOUTS[name]
    times = np.array([0.0, 0.1])
    for sizes, sets in ((SIX, cases.TIME_SETS), (REST, ("absolute", "ns", "uniform"))):
        blobs = [_blob(layout, scans[n], times, ts)[0] for n, ts in zip(sizes, sets)]
        on, off = ctx.batch_empty(len(sizes), max(sizes)), ctx.batch_empty(len(sizes), max(sizes))
        try:
            on.keep_times()
            c_on, c_off = on.upload_records(layout, blobs), off.upload_records(layout, blobs)
            assert c_on.tolist() == c_off.tolist()
            assert _equal(_state(on), _state(off))
            for s, (bl, n) in enumerate(zip(blobs, sizes)):
                want = rref.survivors(layout, bl, n, 0.0)[3]
                got = on.download_times(s)
                assert got.dtype == np.float64 and _same(got, want), (name, s, n)
            assert "no resident times" in str(_refused(api, lambda: off.download_times(0)))
            # a layout without a time field leaves none, and the ingest itself succeeds; so does the switch turned off again
            on.upload_records(dict(layout, time_kind=rref.TIME_NONE), blobs)
            assert "no resident times" in str(_refused(api, lambda: on.download_times(0)))
            on.upload_records(layout, blobs)
            assert len(on.download_times(0)) == c_on[0]
            on.keep_times(False)
            assert "no resident times" in str(_refused(api, lambda: on.download_times(0)))
            on.upload_records(layout, blobs)
            assert "no resident times" in str(_refused(api, lambda: on.download_times(0)))
        finally:
            on.close()
            off.close()


# ---- 2. records: the pass against the ingest-time deskew --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TIMED)
@pytest.mark.parametrize("track", dcases.TRACKS)
def test_records_equal_the_deskewed_ingest_byte_for_byte(api, ctx, scans, name, track):
    layout = cases.LAYOUTS[name]
    blobs, offs, motion = _case(layout, [scans[n] for n in SIX], track, cases.TIME_SETS, WHICHS)
    origins = motion["knot_times"][:, 0] - dcases.track(track)[0][0]
    other = _remotion(dcases.TRACKS[(dcases.TRACKS.index(track) + 1) % len(dcases.TRACKS)], origins, WHICHS[::-1])
    src, dst, ing = (ctx.batch_empty(6, max(SIX)) for _ in range(3))
    wide = ctx.batch_empty(6, max(SIX) + 37)  # another pitch than src's
    try:
        src.keep_times()
        counts = src.upload_records(layout, blobs)
        raw, raw_times = _state(src), [src.download_times(s) for s in range(6)]
        moved = 0.0
        for m, to in ((motion, dst), (other, wide)):  # a second compensation of src, with another track, into another batch
            assert src.deskew(to, offs, **m) is to
            assert ing.upload_records_deskew(layout, blobs, offs, m["knot_times"], m["knot_poses"], m["ref_times"]).tolist() == counts.tolist()
            got, want = _state(to), _state(ing)
            assert [len(p) for p, _ in got] == counts.tolist()
            assert _equal(got, want), (name, track)
            assert all(np.array_equal(r, r0) for (_, r), (_, r0) in zip(got, raw))  # the rings are src's
            assert all(not _bits(p[:, 3]).any() for p, _ in got)
            assert _equal(_state(src), raw) and all(_same(src.download_times(s), raw_times[s]) for s in range(6))  # src is unchanged
            assert "no resident times" in str(_refused(api, lambda: to.download_times(0)))  # dst never holds times
            moved = max(moved, max(float(np.abs(p[:, :3] - q[:, :3]).max()) for (p, _), (q, _) in zip(got, raw) if len(p)))
        assert moved > 0.05  # the tracks move the sensor by decimetres to metres: a pass that ignored them would pass nothing above
        # in place: the same bytes, and compensated points are not compensated again
        assert src.deskew(None, offs, **other) is src
        assert _equal(_state(src), _state(ing))
        assert "no resident times" in str(_refused(api, lambda: src.deskew(None, offs, **other)))
        assert "no resident times" in str(_refused(api, lambda: wide.deskew(dst, offs, **other)))
    finally:
        for b in (src, dst, ing, wide):
            b.close()


# ---- 3. the points against the numpy restatement, given the ingest form's matrices ---------------------------------------------------------
@pytest.mark.parametrize("name", ["velodyne", "rslidar", "ouster"])  # F32, F64 and U32 time fields
def test_points_equal_the_restatement_byte_for_byte(ctx, scans, name):
    layout = cases.LAYOUTS[name]
    sizes = (4096 + 17, 1024, 0, 1025)
    for track, sets in (("k9_neg", ("shuffled", "on_knots", "uniform", "absolute")), ("k256", ("ns", "late", "uniform", "on_knots"))):
        blobs, offs, motion = _case(layout, [scans[n] for n in sizes], track, sets, WHICHS[:4])
        src, dst, ing = (ctx.batch_empty(4, max(sizes)) for _ in range(3))
        try:
            ctx.records_deskew_debug(True)
            ing.upload_records_deskew(layout, blobs, offs, motion["knot_times"], motion["knot_poses"], motion["ref_times"])
            mats = [ctx.records_deskew_matrices(s) for s in range(4)]
            ctx.records_deskew_debug(False)
            src.keep_times()
            src.upload_records(layout, blobs)
            src.deskew(dst, offs, **motion)
            for s, n in enumerate(sizes):
                raw, rings, _, key = rref.survivors(layout, blobs[s], n, 0.0)
                assert _same(src.download_times(s), key)
                pts = dst.download_scan(s)
                assert len(mats[s]) == len(raw) == len(pts)
                assert _same(pts, dref.apply(raw, np.arange(len(raw)), mats[s])), (name, track, s)
                assert np.array_equal(dst.download_rings(s), rings)
        finally:
            ctx.records_deskew_debug(False)
            for b in (src, dst, ing):
                b.close()


# ---- 4. range images ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sensor", [("A", 4, 300), ("C", 5, 1231)])
@pytest.mark.parametrize("table", dcases.COL_TABLES)
def test_ranges_equal_the_deskewed_ingest_byte_for_byte(api, synth, ctx, sensor, table):
    import test_gpu_range_deskew as rd  # sensors A and C and the images are that file's
    _, n_rings, n_cols = sensor
    model = api.SensorModel(n_rings, n_cols, rd.SCALE, rd.MIN_RANGE, *rd._tables(synth, n_rings, n_cols, False))
    images = rd._images(model.cells, 11 + n_rings)  # no return anywhere, a hit everywhere, holes, everything too near
    track = dcases.TRACKS[dcases.COL_TABLES.index(table) + (2 if n_rings == 5 else 0)]
    times, poses = dcases.track(track)
    col = dcases.col_times(times, n_cols, table)
    rt = np.array([dcases.ref_time(times, col, w) for w in ("last_col", "first_knot", "mid", "mid")])
    motion = dict(knot_times=np.tile(times, (4, 1)), knot_poses=np.tile(poses, (4, 1, 1)), ref_times=rt)
    sn = api.Sensor(ctx, model)
    src, dst, ing = (ctx.batch_empty(4, model.cells) for _ in range(3))
    try:
        src.keep_times()
        counts = src.upload_ranges(sn, images)  # a sensor without column times leaves none, and the ingest succeeds
        assert "no resident times" in str(_refused(api, lambda: src.download_times(0)))
        sn.set_col_times(col)
        assert src.upload_ranges(sn, images).tolist() == counts.tolist()
        raw = _state(src)
        for s, im in enumerate(images):
            pts, rings, cols = dref.survivors(model, im)
            assert _same(raw[s][0], pts) and np.array_equal(raw[s][1], rings)
            assert _same(src.download_times(s), col[cols]), (sensor, table, s)
        src.deskew(dst, None, **motion)  # time_offsets=None: the key IS the time
        assert ing.upload_ranges_deskew(sn, images, motion["knot_times"], motion["knot_poses"], rt).tolist() == counts.tolist()
        assert _equal(_state(dst), _state(ing)), (sensor, table)
        assert _equal(_state(src), raw)
        assert counts[1] == model.cells and float(np.abs(dst.download_scan(1)[:, :3] - raw[1][0][:, :3]).max()) > 0.05
        # the deskewed ingest form never leaves times
        src.upload_ranges_deskew(sn, images, motion["knot_times"], motion["knot_poses"], rt)
        assert "no resident times" in str(_refused(api, lambda: src.deskew(dst, None, **motion)))
    finally:
        for b in (src, dst, ing):
            b.close()
        sn.close()


# ---- 5. the identity track leaves the plain bytes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["velodyne_packed", "ouster"])
def test_identity_track_leaves_the_plain_bytes(ctx, scans, name):
    layout = cases.LAYOUTS[name]
    sizes = (4096 + 17, 1024, 0, 1025)
    for K in (2, 7):
        times = np.linspace(0.0, 0.1, K)
        blobs = [_blob(layout, scans[n], times, ts)[0] for n, ts in zip(sizes, ("on_knots", "late", "uniform", "shuffled"))]
        src, dst = ctx.batch_empty(4, max(sizes)), ctx.batch_empty(4, max(sizes))
        try:
            src.keep_times()
            assert src.upload_records(layout, blobs)[0] > 2000
            src.deskew(dst, np.zeros(4), knot_times=np.tile(times, (4, 1)), knot_poses=np.tile(IDENTITY, (4, K, 1)), ref_times=[0.1, 0.0, 0.033, 0.3])
            assert _equal(_state(dst), _state(src))
        finally:
            src.close()
            dst.close()


# ---- 6. batch independence ------------------------------------------------------------------------------------------------------------------
def test_a_scan_does_not_depend_on_its_batch(ctx, scans):
    layout = cases.LAYOUTS["velodyne"]
    n = 4096 + 17
    t_a, p_a = dcases.track("k9_neg")
    p_b = p_a.copy()
    p_b[:, 4:] += np.linspace(0.0, 3.0, len(t_a))[:, None]  # another motion for the other scans of the batch
    mine, off, _ = _blob(layout, scans[n], t_a, "shuffled")
    other = _blob(layout, scans[1025], t_a, "uniform")[0]
    r_a, r_b = cases.ref_time(t_a, "mid"), cases.ref_time(t_a, "last")

    def run(place, count, in_place):
        kp, rt = np.tile(p_b, (count, 1, 1)), np.full(count, r_b)
        kp[place], rt[place] = p_a, r_a
        blobs = [other] * count
        blobs[place] = mine
        src, dst = ctx.batch_empty(count, n), ctx.batch_empty(count, n + 5 * count)
        try:
            src.keep_times()
            src.upload_records(layout, blobs)
            out = src.deskew(None if in_place else dst, np.full(count, off), knot_times=np.tile(t_a, (count, 1)), knot_poses=kp, ref_times=rt)
            return out.download_scan(place), out.download_rings(place)
        finally:
            src.close()
            dst.close()

    alone = run(0, 1, False)
    assert len(alone[0]) == len(rref.survivors(layout, mine, n)[0]) > 2000
    for place, count, in_place in ((0, 3, False), (2, 3, True), (0, 7, True), (6, 7, False), (3, 7, False), (0, 1, True)):
        got = run(place, count, in_place)
        assert _same(got[0], alone[0]) and np.array_equal(got[1], alone[1]), (place, count, in_place)


# ---- 7. refusals leave dst as it was --------------------------------------------------------------------------------------------------------
def _with_times(layout, scan, times, survivor_values):
    """A blob of `scan` on the uniform time set with the time of survivor number i replaced by v for every (i, v)."""
    xyz, ring, inten, dropped = scan
    rel, origin = cases.rel_times(times, len(xyz), "uniform")
    tf = cases.garbage_times(layout, cases.encode(layout, rel, origin)[0], dropped)
    kept = np.nonzero(~dropped)[0]
    for i, v in survivor_values:
        tf[kept[i]] = v
    return rref.pack(layout, xyz, tf, ring, inten, seed=len(xyz))


def test_time_refusals_follow_the_prediction_and_leave_dst_as_it_was(api, ctx, scans):
    layout = cases.LAYOUTS["rslidar"]
    times, poses = dcases.track("k9_neg")
    sizes = (1025, 65, 1023, 4096 + 17)
    motion = dict(knot_times=np.tile(times, (4, 1)), knot_poses=np.tile(poses, (4, 1, 1)), ref_times=np.full(4, times[-1]))
    good = [_blob(layout, scans[n], times, "uniform")[0] for n in sizes]
    sets = {
        # the late time set is served with the plain offsets (0.2 s behind the last knot) and refused once the offset adds 0.31 s
        "late": ([_blob(layout, scans[n], times, "late")[0] for n in sizes], np.array([0.0, 0.31, 0.0, 0.31])),
        # survivors before the first knot in scans 1 (two) and 2 (one), by the field and by the offset
        "early": ([good[0], _with_times(layout, scans[65], times, [(3, times[0] - 1e-6), (20, times[0] - 1e-6)]), _with_times(layout, scans[1023], times, [(700, times[0] - 1.0)]),
                   good[3]], np.zeros(4)),
        "early_offset": (good, np.array([0.0, 0.0, 0.0, -0.05])),  # half of the sweep of scan 3 (its first records are dropped ones)
        # 0.5001 s behind the last knot in the last tile of the longest scan; a NaN survivor time
        "far": ([good[0], good[1], good[2], _with_times(layout, scans[4096 + 17], times, [(-1, times[-1] + 0.5001)])], np.zeros(4)),
        "nan": ([_with_times(layout, scans[1025], times, [(500, np.nan)]), good[1], good[2], good[3]], np.zeros(4)),
    }
    src, dst = ctx.batch_empty(4, max(sizes)), ctx.batch_empty(4, max(sizes))
    try:
        src.keep_times()
        dst.upload_records(layout, [bl[:32 * 40] for bl in good])
        dst_before = _state(dst)
        for what, (blobs, offs) in sets.items():
            src.upload_records(layout, blobs)
            before, keys = _state(src), [src.download_times(s) for s in range(4)]
            bad = [int(rref.bad_times(times, k + o).sum()) for k, o in zip(keys, offs)]
            assert any(bad), what
            first = next(i for i, x in enumerate(bad) if x)
            for to in (dst, src):  # into another batch, then in place
                e = _refused(api, lambda: src.deskew(to, offs, **motion))
                assert e.status.tolist() == [int(x > 0) for x in bad], (what, bad)
                assert "scan %d has %d survivors" % (first, bad[first]) in str(e) and "0.5 s" in str(e) and "unchanged" in str(e), (what, str(e))
                assert _equal(_state(dst), dst_before) and _equal(_state(src), before)
                assert all(_same(src.download_times(s), keys[s]) for s in range(4))  # src is still raw and can be compensated
            if what == "late":  # served without the offsets, as the ingest form serves it
                src.deskew(dst, None, **motion)
                ing = ctx.batch_empty(4, max(sizes))
                try:
                    ing.upload_records_deskew(layout, blobs, np.zeros(4), motion["knot_times"], motion["knot_poses"], motion["ref_times"])
                    assert _equal(_state(dst), _state(ing))
                finally:
                    ing.close()
                dst.upload_records(layout, [bl[:32 * 40] for bl in good])
                assert _equal(_state(dst), dst_before)
    finally:
        src.close()
        dst.close()


def test_host_refusals_come_with_a_text_and_leave_dst_as_it_was(api, ctx, scans):
    L = api.lib()
    layout = cases.LAYOUTS["velodyne"]
    times, poses = dcases.track("k4_short")
    sizes = (1025, 65, 1023, 1024)
    blobs = [_blob(layout, scans[n], times, "uniform")[0] for n in sizes]
    motion = dict(knot_times=np.tile(times, (4, 1)), knot_poses=np.tile(poses, (4, 1, 1)), ref_times=np.full(4, times[-1]))
    offs = np.zeros(4)
    src, dst, plain = ctx.batch_empty(4, 1025), ctx.batch_empty(4, 1025), ctx.batch_empty(4, 1025)
    other_n = ctx.batch_empty(3, 1025)
    shared = small = None
    try:
        src.keep_times()
        counts = src.upload_records(layout, blobs)
        small = ctx.batch_empty(4, int(counts.max()) - 1)
        small.upload_records(layout, [bl[:32 * 40] for bl in blobs])
        plain.upload_records(layout, blobs)
        dst.upload_records(layout, [bl[:32 * 40] for bl in blobs])
        before = {id(b): _state(b) for b in (src, dst, small)}
        keys = [src.download_times(s) for s in range(4)]

        def unchanged():
            assert all(_equal(_state(b), before[id(b)]) for b in (src, dst, small))
            assert all(_same(src.download_times(s), keys[s]) for s in range(4))

        def says(word, call):
            assert word in str(_refused(api, call)), word

        says("no resident times", lambda: plain.deskew(dst, offs, **motion))  # the switch was off at its ingest
        says("dst was created for", lambda: src.deskew(small, offs, **motion))
        says(str(int(counts.max())), lambda: src.deskew(small, offs, **motion))
        says("different numbers of scans", lambda: src.deskew(other_n, offs, **motion))
        says("time_offsets[2]", lambda: src.deskew(dst, np.array([0.0, 0.0, np.inf, 0.0]), **motion))
        # every motion refusal of the range-image path, by its host function
        says("n_knots", lambda: src.deskew(dst, offs, knot_times=np.zeros((4, 1)), knot_poses=np.tile(IDENTITY, (4, 1, 1)), ref_times=np.zeros(4)))
        kt = motion["knot_times"].copy()
        kt[3, 2] = kt[3, 1]
        e = _refused(api, lambda: src.deskew(dst, offs, knot_times=kt, knot_poses=motion["knot_poses"], ref_times=motion["ref_times"]))
        assert "increasing" in str(e) and "scan 3" in str(e)
        says("0.5 s", lambda: src.deskew(dst, offs, **dict(motion, ref_times=np.full(4, times[-1] + 0.6))))
        says("before the first knot", lambda: src.deskew(dst, offs, **dict(motion, ref_times=np.full(4, times[0] - 1e-3))))
        says("not finite", lambda: src.deskew(dst, offs, **dict(motion, ref_times=np.array([0.0, np.nan, 0.0, 0.0]))))
        m, keep_m = api.sweep_motion(4, motion["knot_times"], motion["knot_poses"], motion["ref_times"])
        assert L.locgpu_batch_deskew(src._h, dst._h, None, None, None) == INVALID and b"motion is NULL" in L.locgpu_last_error(ctx._h)
        m_null = api.SweepMotionC(m.n_knots, 0, m.knot_times, None, m.ref_times)
        assert L.locgpu_batch_deskew(src._h, dst._h, None, ctypes.byref(m_null), None) == INVALID and b"NULL array" in L.locgpu_last_error(ctx._h)
        assert L.locgpu_batch_deskew(src._h, None, None, ctypes.byref(m), None) == INVALID and b"NULL batch" in L.locgpu_last_error(ctx._h)
        assert L.locgpu_batch_deskew(None, dst._h, None, ctypes.byref(m), None) == INVALID and b"NULL batch" in L.locgpu_last_error(ctx._h)
        unchanged()
        # a shared-source batch, as source or destination, and its switch
        shared = ctx.batch_shared(np.ones((8, 3), np.float32), 4)
        says("shared-source", lambda: src.deskew(shared, offs, **motion))
        says("shared-source", lambda: shared.deskew(dst, offs, **motion))
        says("shared-source", lambda: shared.keep_times())
        # an alignment begun and not ended, on either batch
        ctx.icp_set_target(plain.download_scan(0)[:, :3])
        opts = api.icp_opts(method=api.P2P, max_iteration=2)
        for busy in (src, dst):
            ctx.icp_align_batch_begin(busy, np.tile(IDENTITY, (4, 1)), opts)
            try:
                says("begun", lambda: src.deskew(dst, offs, **motion))
                says("begun", lambda: busy.keep_times(False))
                if busy is src:
                    says("begun", lambda: src.download_times(0))
            finally:
                ctx.align_batch_end(busy)
        unchanged()
        # whatever drops the rings drops the times: a preprocess into the batch, an upload with the switch off, a host upload
        probe = ctx.batch_empty(4, 1025)
        try:
            probe.keep_times()
            probe.upload_records(layout, blobs)
            assert len(probe.download_times(0)) == counts[0]
            src.preprocess(0.5, out=probe)
            says("no resident times", lambda: probe.deskew(dst, offs, **motion))
            probe.upload_records(layout, blobs)
            probe.upload_async([p for p, _ in before[id(src)]])
            probe.upload_wait()
            says("no resident times", lambda: probe.download_times(0))
            probe.upload_records(layout, blobs)
            probe.keep_times(False)
            probe.upload_records(layout, blobs)
            says("no resident times", lambda: probe.deskew(dst, offs, **motion))
        finally:
            probe.close()
        unchanged()
        # and after all of them the call still works
        src.deskew(dst, offs, **motion)
        plain.upload_records_deskew(layout, blobs, offs, motion["knot_times"], motion["knot_poses"], motion["ref_times"])
        assert _equal(_state(dst), _state(plain))
    finally:
        for b in (src, dst, plain, other_n, small, shared):
            if b is not None:
                b.close()


# ---- 8. downstream: the feature picker on the compensated batch -------------------------------------------------------------------------------
def test_loam_picker_downstream_equals_the_deskewed_ingest(api, synth, ctx):
    n_rings, n_cols = 4, 300
    model = api.SensorModel(n_rings, n_cols, 0.002, 4.0, *synth.sensor_tables(n_rings, n_cols))
    image = synth.make_range_image(3, model).reshape(-1)
    raw_pts, rings, cols = dref.survivors(model, image)
    times, poses = dcases.track("k33_small")  # 1.5 m and 3.2 mrad over the sweep: rings stay rings
    col = dcases.col_times(times, n_cols, "uniform")
    layout = cases.LAYOUTS["velodyne"]
    blob = rref.pack(layout, raw_pts[:, :3], col[cols].astype(np.float32), rings, np.arange(len(rings)) % 200)
    blobs = [blob, blob[:32 * 500], blob[:32 * 777], blob]
    motion = dict(knot_times=np.tile(times, (4, 1)), knot_poses=np.tile(poses, (4, 1, 1)), ref_times=[cases.ref_time(times, w) for w in ("last", "mid", "first_knot", "mid")])
    src, dst, ing = (ctx.batch_empty(4, 1200) for _ in range(3))
    edge, surf = ctx.batch_empty(4, 4 * 6 * 20), ctx.batch_empty(4, 1200)
    try:
        ing.upload_records_deskew(layout, blobs, np.zeros(4), motion["knot_times"], motion["knot_poses"], motion["ref_times"])
        ne0, ns0, st0 = ing.loam_extract_resident(4, edge, surf)
        want = [(edge.download_scan(s), surf.download_scan(s)) for s in range(4)]
        assert ne0[0] > 0 and ns0[0] > 0
        src.keep_times()
        src.upload_records(layout, blobs)
        src.deskew(dst, np.zeros(4), **motion)
        ne, ns, st = dst.loam_extract_resident(4, edge, surf)
        assert ne.tolist() == ne0.tolist() and ns.tolist() == ns0.tolist() and st.tolist() == st0.tolist()
        for s in range(4):
            assert _same(edge.download_scan(s), want[s][0]) and _same(surf.download_scan(s), want[s][1]), s
    finally:
        for b in (src, dst, ing, edge, surf):
            b.close()


# ---- 9. composed: ingest once, align, motion from the results, compensate ---------------------------------------------------------------------
def test_ingest_align_motion_from_poses_deskew_equals_the_deskewed_ingest(api, synth, ctx):
    layout = cases.LAYOUTS["velodyne"]
    n, period = 3, 0.1
    stamps = 100.0 + period * np.arange(n)  # start-stamped sweeps
    blobs, inits = [], []
    for i in range(n):
        xyz = np.ascontiguousarray(synth.make_scan(3 + i, subsample=3000, crop_half=36.0)[:, :3], dtype=np.float32)
        t = np.linspace(0.0, period, len(xyz)).astype(np.float32)  # seconds from the sweep's stamp
        blobs.append(rref.pack(layout, xyz, t, np.arange(len(xyz)) % 16, None, seed=i))
        inits.append(synth.make_pose(3 + i)[1])
    src, dst, ing, flt = (ctx.batch_empty(n, 3000) for _ in range(4))
    try:
        src.keep_times()
        counts = src.upload_records(layout, blobs)
        assert counts.min() > 500
        raw = _state(src)
        ctx.icp_set_target(synth.make_local_map(20000, 3, half=40.0))
        src.preprocess(0.5, out=flt)  # the alignment runs on a filtered copy: src stays raw, with its times
        out_poses, stats = ctx.icp_align_batch(flt, np.array(inits), api.icp_opts(method=api.P2P, max_iteration=5))
        assert np.isfinite(out_poses).all() and len(stats) == n
        kt, kp = api.motion_from_poses(out_poses, stamps)
        assert kt.shape == (n, 3) and kp.shape == (n, 3, 7) and np.isfinite(kp).all()
        assert _same(kp[:, 1], np.ascontiguousarray(out_poses, dtype=np.float64)) and _same(kt[:, 1], stamps)
        rt = stamps + period  # each sweep expressed in the sensor frame of its end
        src.deskew(dst, stamps, knot_times=kt, knot_poses=kp, ref_times=rt)
        assert ing.upload_records_deskew(layout, blobs, stamps, kt, kp, rt).tolist() == counts.tolist()
        assert _equal(_state(dst), _state(ing))
        assert _equal(_state(src), raw)
        assert any(not _same(p, q) for (p, _), (q, _) in zip(_state(dst), raw))
    finally:
        for b in (src, dst, ing, flt):
            b.close()


# ---- 10. profiling ----------------------------------------------------------------------------------------------------------------------------
def test_kernel_times_are_reported(ctx, scans):
    layout = cases.LAYOUTS["ouster"]
    times, poses = dcases.track("k2")
    sizes = (4096 + 17, 1024, 0, 1025)
    blobs = [_blob(layout, scans[n], times, "ns")[0] for n in sizes]
    src = ctx.batch_empty(4, max(sizes))
    try:
        src.keep_times()
        src.upload_records(layout, blobs)
        other = (ctx.records_ingest_times(), ctx.range_ingest_times(), ctx.range_deskew_times())
        ctx.profile_enable(True)
        src.deskew(None, np.zeros(4), knot_times=np.tile(times, (4, 1)), knot_poses=np.tile(poses, (4, 1, 1)), ref_times=np.full(4, times[-1]))
        check_ms, move_ms = ctx.batch_deskew_times()
        print("resident deskew: check kernel %.3f ms, move kernel %.3f ms" % (check_ms, move_ms))
        assert 0 < check_ms < 1e3 and 0 < move_ms < 1e3
        assert (ctx.records_ingest_times(), ctx.range_ingest_times(), ctx.range_deskew_times()) == other
    finally:
        ctx.profile_enable(False)
        src.close()
