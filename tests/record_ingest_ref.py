"""The point-record ingest restated in numpy (include/locgpu.h, "Point-record ingest"): packing driver-style point
records into a blob, reading the fields back where a layout says they are, CloudConver::Conver's two rules
(LocUtils/src/subscriber/cloud_subscriber.cpp:7-29 and :31-58) and the point's time. Test infrastructure: what
locgpu_batch_upload_records[_deskew] and locgpu_cloud_upload_records[_deskew] are held to.

The matrices and their application are range_deskew_ref's, unchanged: ``range_deskew_ref.matrices(knot_times, knot_poses, tp, ref_time,
dtype)`` already is the per-point rule with the points' times in place of the column table, and ``range_deskew_ref.apply(raw,
np.arange(n), mats)`` applies matrix i to point i."""
import numpy as np

TIME_NONE, TIME_F32, TIME_F64, TIME_U32 = 0, 1, 2, 3
RING_NONE, RING_U8, RING_U16 = 0, 1, 2
INTENSITY_NONE, INTENSITY_F32, INTENSITY_U8 = 0, 1, 2
TIME_DTYPE = {TIME_F32: "<f4", TIME_F64: "<f8", TIME_U32: "<u4"}
RING_DTYPE = {RING_U8: "u1", RING_U16: "<u2"}
INTENSITY_DTYPE = {INTENSITY_F32: "<f4", INTENSITY_U8: "u1"}
DEFAULTS = dict(xyz_offset=0, time_offset=0, time_kind=TIME_NONE, ring_offset=0, ring_kind=RING_NONE, intensity_offset=0, intensity_kind=INTENSITY_NONE,
                min_range=4.0, time_scale=1.0)


def full(layout):
    """A layout given as plain data with every field present."""
    d = dict(DEFAULTS)
    d.update(layout)
    return d


def _fields(layout):
    """(name, offset, dtype) of the fields a layout holds besides xyz."""
    L = full(layout)
    out = []
    if L["time_kind"] != TIME_NONE:
        out.append(("time", L["time_offset"], np.dtype(TIME_DTYPE[L["time_kind"]])))
    if L["ring_kind"] != RING_NONE:
        out.append(("ring", L["ring_offset"], np.dtype(RING_DTYPE[L["ring_kind"]])))
    if L["intensity_kind"] != INTENSITY_NONE:
        out.append(("intensity", L["intensity_offset"], np.dtype(INTENSITY_DTYPE[L["intensity_kind"]])))
    return out


def pack(layout, xyz, time=None, ring=None, intensity=None, seed=1):
    """A blob (uint8 [n * stride]) of n records: xyz [n, 3] float32 and the fields the layout holds, each value cast to its field's
    type; every byte no field covers is filled from a seeded byte pattern, not zeros."""
    L = full(layout)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n, stride = len(xyz), L["stride_bytes"]
    blob = np.random.default_rng(seed).integers(0, 256, (n, stride), dtype=np.uint8)
    blob[:, L["xyz_offset"]:L["xyz_offset"] + 12] = np.ascontiguousarray(xyz.astype("<f4")).view(np.uint8).reshape(n, 12)
    values = dict(time=time, ring=ring, intensity=intensity)
    for name, off, dt in _fields(L):
        v = values[name]
        v = np.zeros(n, dt) if v is None else np.asarray(v).astype(dt)
        blob[:, off:off + dt.itemsize] = np.ascontiguousarray(v).view(np.uint8).reshape(n, dt.itemsize)
    return blob.reshape(-1)


def field(layout, blob, n, off, dtype):
    """n values of `dtype` at byte offset `off` of every record, read as memcpy would read them."""
    L = full(layout)
    dt = np.dtype(dtype)
    rows = np.frombuffer(bytes(blob), np.uint8, n * L["stride_bytes"]).reshape(n, L["stride_bytes"])
    return np.frombuffer(np.ascontiguousarray(rows[:, off:off + dt.itemsize]).tobytes(), dt)


def keep_mask(layout, blob, n):
    """Conver's two rules on the raw points, float32 arithmetic: finite, and not sqrtf((x*x + y*y) + z*z) < min_range."""
    L = full(layout)
    F = np.float32
    x, y, z = (field(L, blob, n, L["xyz_offset"] + 4 * i, "<f4") for i in range(3))
    with np.errstate(all="ignore"):
        d = np.sqrt((x * x + y * y) + z * z)
        return np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(d < F(L["min_range"]))


def survivors(layout, blob, n, time_offset=0.0):
    """(raw points [m, 4] float32 with lane w +0, ring bytes [m] uint8, intensities [m] float32, times [m] float64) of a blob's
    survivors in input order. Time: (double)field * time_scale + time_offset, two float64 operations; zeros without a time field."""
    L = full(layout)
    keep = keep_mask(L, blob, n)
    m = int(keep.sum())
    raw = np.zeros((m, 4), np.float32)
    for i in range(3):
        raw[:, i] = field(L, blob, n, L["xyz_offset"] + 4 * i, "<f4")[keep]
    rings, inten, times = np.zeros(m, np.uint8), np.zeros(m, np.float32), np.zeros(m, np.float64)
    for name, off, dt in _fields(L):
        v = field(L, blob, n, off, dt)[keep]
        if name == "ring":
            rings = v.astype(np.uint8)  # (uint8_t)ring: the low byte
        elif name == "intensity":
            inten = v.astype(np.float32)
        else:
            with np.errstate(all="ignore"):
                times = v.astype(np.float64) * np.float64(L["time_scale"]) + np.float64(time_offset)
    return raw, rings, inten, times


def bad_times(knot_times, tp):
    """The header's time refusal per survivor: not finite, before the first knot, more than 0.5 s behind the last."""
    t, tp = np.asarray(knot_times, np.float64), np.asarray(tp, np.float64)
    with np.errstate(all="ignore"):
        return ~np.isfinite(tp) | (tp < t[0]) | (tp - t[-1] > 0.5)
