"""The numpy restatement of the point-record ingest (tests/record_ingest_ref.py) checked against itself and against the range-image
restatement (tests/range_deskew_ref.py), without a GPU: packing and reading back round-trip for every layout; records made of a range
image's survivors reproduce the deskewed decode of that image byte for byte, so the two restatements are one rule; and the unit the
GPU test measures the device's matrices in is printed per track."""
import numpy as np
import pytest

import range_deskew_cases as dcases
import range_deskew_ref as dref
import record_ingest_cases as cases
import record_ingest_ref as rref


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32)


@pytest.mark.parametrize("name", list(cases.LAYOUTS))
def test_pack_then_survivors_round_trips(name):
    layout = rref.full(cases.LAYOUTS[name])
    for n in (0, 1, 65, 1025):
        xyz, ring, inten, dropped = cases.scan(n, 3 + n)
        times, _ = dcases.track("k9_neg")
        has_time = layout["time_kind"] != rref.TIME_NONE
        tf, off = cases.encode(layout, *cases.rel_times(times, n, "shuffled")) if has_time else (None, 0.0)
        if has_time:
            tf = cases.garbage_times(layout, tf, dropped)
        blob = rref.pack(layout, xyz, tf, ring, inten, seed=n)
        assert blob.dtype == np.uint8 and blob.size == n * layout["stride_bytes"]
        keep = rref.keep_mask(layout, blob, n)
        assert np.array_equal(keep, ~dropped)  # the generator's drops are exactly the rule's
        if n > 1000:
            assert 0.2 < dropped.mean() < 0.4
        raw, rings, got_i, tp = rref.survivors(layout, blob, n, off)
        assert np.array_equal(_bits(raw[:, :3]), _bits(xyz[keep])) and not _bits(raw[:, 3]).any()
        if layout["ring_kind"] != rref.RING_NONE:
            assert rings.dtype == np.uint8 and np.array_equal(rings, (ring[keep] & 0xFF).astype(np.uint8))
            if n > 300:
                assert (ring[keep] > 255).any()
        else:
            assert not rings.any()
        if layout["intensity_kind"] != rref.INTENSITY_NONE:
            assert np.array_equal(got_i, inten[keep])
        if has_time:
            assert np.isfinite(tp).all() and not rref.bad_times(times, tp).any()
            assert np.array_equal(tp, tf[keep].astype(np.float64) * layout["time_scale"] + off)
        # the bytes no field covers are not zeros
        covered = set(range(layout["xyz_offset"], layout["xyz_offset"] + 12))
        for _, off_f, dt in rref._fields(layout):
            covered |= set(range(off_f, off_f + dt.itemsize))
        free = sorted(set(range(layout["stride_bytes"])) - covered)
        if n > 100 and free:
            assert len(np.unique(blob.reshape(n, -1)[:, free[0]])) > 50


def test_exactly_four_metres_is_kept():
    layout = cases.LAYOUTS["xyz12"]
    below = np.nextafter(np.float32(4.0), np.float32(0.0))
    xyz = np.array([[4.0, 0, 0], [0, below, 0], [0, 0, -4.0], [np.nan, 9, 9], [9, np.inf, 9], [9, 9, -np.inf]], np.float32)
    assert rref.keep_mask(layout, rref.pack(layout, xyz), 6).tolist() == [True, False, True, False, False, False]


@pytest.mark.parametrize("sensor", [(4, 300), (5, 1231)])
def test_records_of_a_range_image_reproduce_its_deskewed_decode(api, synth, sensor):
    n_rings, n_cols = sensor
    model = api.SensorModel(n_rings, n_cols, 0.002, 4.0, *synth.sensor_tables(n_rings, n_cols))
    rng = np.random.default_rng(n_cols)
    image = rng.integers(1500, 65536, model.cells).astype(np.uint16)
    image[rng.random(model.cells) < 0.2] = 0
    raw, rings, cols = dref.survivors(model, image)
    times, poses = dcases.track("k9_neg")
    col_time = dcases.col_times(times, n_cols, "rolled")
    r = dcases.ref_time(times, col_time, "mid")
    want = dref.apply(raw, cols, dref.matrices(times, poses, col_time, r))
    layout = cases.LAYOUTS["rslidar"]
    blob = rref.pack(layout, raw[:, :3], col_time[cols], rings, None)
    got_raw, got_rings, _, tp = rref.survivors(layout, blob, len(raw))
    assert len(got_raw) == len(raw) > 0 and np.array_equal(got_rings, rings) and np.array_equal(tp, col_time[cols])
    got = dref.apply(got_raw, np.arange(len(got_raw)), dref.matrices(times, poses, tp, r))
    assert np.array_equal(_bits(got), _bits(want))
    assert float(np.abs(got[:, :3] - raw[:, :3]).max()) > 0.05


def test_unit_of_the_float64_restatement():
    """Printed per track: the float64 restatement's worst deviation from the longdouble one over all point-time sets and reference times,
    in multiples of eps * max(1, max ||t||). Measured on x86-64: k2 0.86, k9_neg 0.78, k33_small 0.95, k5_equalq 0.67, k4_short 0.92,
    k256 0.95; single sets go as low as 0.23, which is why the unit is the maximum over the sets."""
    for track in dcases.TRACKS:
        u, per = cases.unit(track)
        print("%-10s unit %.2f  (%s)" % (track, u, ", ".join("%s %.2f" % kv for kv in per.items())))
        assert 0.1 < u < 4.0, (track, u)  # an error of a few eps: the restatement is float64 arithmetic and nothing coarser
