"""The layouts, scans and point-time sets the point-record ingest is tested on, shared by test_record_ingest_ref.py (no GPU) and
test_gpu_record_ingest.py, and the unit the device's matrices are measured in. Tracks are range_deskew_cases.track's.

Layouts: the reference's three record types as PCL lays them out (point_types.h:99-169), a packed 22-byte Velodyne record with a
float32 at offset 18, a 12-byte xyz-only record and a 64-byte record with a U8 ring and a U8 intensity.
Scans: about 30 % of the records dropped — NaN, +Inf and -Inf in x, y or z separately, ranges below 4 m (exactly 4.0 is kept), a run
of drops across every multiple of 256 — and every dropped record carries a NaN or huge time.
Point times of a track, seconds from the first knot, before a layout's encoding:
  uniform   the float32 offsets of a sweep over the knot span
  ns        whole nanoseconds over the span
  absolute  uniform, on a clock that reads 1.7e9 s at the first knot (the knot times are on that clock too)
  on_knots  entries exactly on knot times, the first and last included
  late      a seventh of the entries 0.2 s behind the last knot
  shuffled  uniform permuted: input order is not time order
Encoding (encode): an F32 field holds float32(seconds) and the clock's origin goes into time_offsets (the Velodyne mapping); a U32
field holds rint(seconds * 1e9) with time_scale 1e-9 (Ouster); an F64 field holds seconds + origin, time offset 0 (RoboSense)."""
import numpy as np

import range_deskew_cases as dcases
import range_deskew_ref as dref
import record_ingest_ref as rref

LAYOUTS = {
    "velodyne": dict(stride_bytes=32, xyz_offset=0, intensity_offset=16, intensity_kind=rref.INTENSITY_F32, time_offset=20, time_kind=rref.TIME_F32, ring_offset=24,
                     ring_kind=rref.RING_U16),
    "rslidar": dict(stride_bytes=32, xyz_offset=0, intensity_offset=16, intensity_kind=rref.INTENSITY_F32, ring_offset=20, ring_kind=rref.RING_U16, time_offset=24,
                    time_kind=rref.TIME_F64),
    "ouster": dict(stride_bytes=48, xyz_offset=0, intensity_offset=16, intensity_kind=rref.INTENSITY_F32, time_offset=20, time_kind=rref.TIME_U32, time_scale=1e-9,
                   ring_offset=26, ring_kind=rref.RING_U8),
    "velodyne_packed": dict(stride_bytes=22, xyz_offset=0, intensity_offset=12, intensity_kind=rref.INTENSITY_F32, ring_offset=16, ring_kind=rref.RING_U16,
                            time_offset=18, time_kind=rref.TIME_F32),
    "xyz12": dict(stride_bytes=12, xyz_offset=0),
    "wide64": dict(stride_bytes=64, xyz_offset=7, ring_offset=33, ring_kind=rref.RING_U8, intensity_offset=63, intensity_kind=rref.INTENSITY_U8, time_offset=41,
                   time_kind=rref.TIME_F64),
}
READY = {"velodyne": "LAYOUT_VELODYNE", "rslidar": "LAYOUT_RSLIDAR", "ouster": "LAYOUT_OUSTER", "velodyne_packed": "LAYOUT_VELODYNE_PACKED"}  # api's names
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4096 + 17)
TIME_SETS = ("uniform", "ns", "absolute", "on_knots", "late", "shuffled")
EPOCH = 1.7e9


def scan(n, seed):
    """(xyz [n, 3] float32, ring [n], intensity [n], dropped [n] bool): points at 4.5 .. 60 m with about 30 % dropped as the module
    text says. `dropped` is what the generator meant to drop; the restatement's keep rule is the judge."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    xyz = (d * rng.uniform(4.5, 60.0, (n, 1))).astype(np.float32)
    how = rng.random(n)
    idx = np.arange(n)
    run = np.zeros(n, bool)
    for m in range(256, n + 256, 256):  # a run across every multiple of 256 (and so of 1024 and 4096)
        run[max(m - 20, 0):min(m + 21, n)] = True
    run[:int(n * 0.04)] = True
    bad = (how < 0.07) | run
    near = ~bad & (how < 0.14)
    xyz[near] = (d[near] * rng.uniform(0.1, 3.99, (int(near.sum()), 1))).astype(np.float32)
    lane = idx % 3
    what = (idx // 3) % 3
    for k, val in enumerate((np.nan, np.inf, -np.inf)):
        for ln in range(3):
            sel = bad & (what == k) & (lane == ln)
            xyz[sel, ln] = val
    if n > 8:  # exactly 4.0 is kept, the float32 below it is not
        keepers = np.nonzero(~bad & ~near)[0]
        xyz[keepers[0]] = (4.0, 0.0, 0.0)
        xyz[keepers[1]] = (0.0, np.nextafter(np.float32(4.0), np.float32(0.0)), 0.0)
        near[keepers[1]] = True
    ring = rng.integers(0, 300, n)  # above 255: a U16 ring keeps its low byte
    intensity = rng.integers(0, 256, n).astype(np.float32)
    return xyz, ring, intensity, bad | near


def rel_times(times, n, name, seed=5):
    """(seconds from the first knot [n] float64, the clock's origin) of one time set on a track with knot times `times` (first knot 0)."""
    K, span = len(times), times[-1] - times[0]
    t = np.linspace(0.0, span, n).astype(np.float32).astype(np.float64) if n else np.zeros(0)
    origin = 0.0
    if name == "ns":
        t = np.rint(np.linspace(0.0, span, n) * 1e9) * 1e-9
    elif name == "absolute":
        origin = EPOCH
    elif name == "on_knots" and n:
        at = np.unique(np.linspace(0, n - 1, min(K, n)).astype(int))
        t[at] = times[np.linspace(0, K - 1, len(at)).astype(int)]
        if n >= 2:
            assert t[0] == times[0] and t[-1] == times[-1]
    elif name == "late":
        t[::7] = span + 0.2
    elif name == "shuffled":
        t = t[np.random.default_rng(seed).permutation(n)]
    elif name not in ("uniform", "on_knots"):
        raise KeyError(name)
    return t, origin


def encode(layout, rel, origin):
    """(time field values, time_offset) that put the times rel + origin into a layout's time field."""
    kind = rref.full(layout)["time_kind"]
    if kind == rref.TIME_F32:
        return rel.astype(np.float32), origin
    if kind == rref.TIME_U32:
        return np.rint(rel * 1e9).astype(np.uint32), origin
    if kind == rref.TIME_F64:
        return rel + origin, 0.0
    raise KeyError(kind)


def garbage_times(layout, field_values, dropped):
    """The time field with every dropped record's entry replaced by garbage: NaN or huge."""
    v = np.array(field_values)
    i = np.nonzero(dropped)[0]
    if v.dtype.kind == "f":
        v[i[::2]] = np.nan
        v[i[1::2]] = 3e38 if v.dtype == np.float32 else 1e300
    else:
        v[i] = 0xFFFFFFFF
    return v


def ref_time(times, which):
    return {"last": times[-1], "first_knot": times[0], "mid": times[0] + 0.537 * (times[-1] - times[0])}[which]


REF_TIMES = ("last", "first_knot", "mid")


def unit(track, n=300):
    """range_deskew_cases.unit's rule with the point-time sets above: the largest deviation of the float64 restatement's matrices from
    the longdouble restatement's over every time set and reference time of `track`, in multiples of range_deskew_cases.scale().
    Returns (the unit, {time set: its own worst})."""
    times, poses = dcases.track(track)
    per = {}
    for name in TIME_SETS:
        rel, origin = rel_times(times, n, name)
        tp, kt = rel + origin, times + origin
        worst = 0.0
        for which in REF_TIMES:
            r = ref_time(kt, which)
            m64 = dref.matrices(kt, poses, tp, r, np.float64)
            m80 = dref.matrices(kt, poses, tp, r, np.longdouble)
            worst = max(worst, float(np.abs(m64.astype(np.longdouble) - m80).max()))
        per[name] = worst / dcases.scale(poses)
    return max(per.values()), per
