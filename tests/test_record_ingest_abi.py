"""The point-record ingest on the host side: its entry points are exported by liblocgpu.so, declared in include/locgpu.h and bound in
loc_lib_amd/api.py with the header's argument counts; each comment cites CloudConver::Conver and math::PoseInterp; every refusal of
the layout, which needs neither a handle nor a device, comes back as LOCGPU_ERR_INVALID with a text; PointLayoutC marshals field for
field."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import record_ingest_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_batch_upload_records", "locgpu_batch_upload_records_deskew", "locgpu_cloud_upload_records", "locgpu_cloud_upload_records_deskew",
         "locgpu_records_deskew_debug", "locgpu_records_deskew_matrices", "locgpu_records_ingest_times")
INVALID = -1  # LOCGPU_ERR_INVALID


def test_header_library_and_binding_agree(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        m = re.search(r"LOCGPU_API\s+int\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert hasattr(L, name) and name in api.ABI_SYMBOLS, name
        assert len(getattr(L, name).argtypes) == len(args.split(",")), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        above = header[:m.start()]
        comment = above[above.rindex("/*"):]
        for cite in ("math_utils.h:470-517", "cloud_subscriber.cpp"):
            assert cite in comment, (name, cite)
    for cls, method in ((api.Batch, "upload_records"), (api.Batch, "upload_records_deskew"), (api.Cloud, "upload_records"), (api.Cloud, "upload_records_deskew"),
                        (api.Context, "records_deskew_debug"), (api.Context, "records_deskew_matrices"), (api.Context, "records_ingest_times")):
        assert callable(getattr(cls, method))
    # the block stands directly behind the deskewed range-image block and carries the definition
    start = header.index("---- Point-record ingest")
    assert header.index("locgpu_range_deskew_times(") < start < header.index("locgpu_submap_create(")
    block = header[start:header.index("locgpu_batch_upload_records(")]
    for word in ("memcpy", "little-endian", "(uint8_t)ring", "IN INPUT ORDER", "two IEEE double operations", "RAW point", "Out of scope", "big-endian",
                 "strides above 64", "exactly as it was", "0.5", "overlaps xyz", "math_utils.h:470-517", "cloud_subscriber.cpp:7-29", "point_types.h"):
        assert word in block, word
    # the enumerators and the struct the binding hands over are the header's
    for name, value in (("TIME_NONE", 0), ("TIME_F32", 1), ("TIME_F64", 2), ("TIME_U32", 3), ("RING_NONE", 0), ("RING_U8", 1), ("RING_U16", 2),
                        ("INTENSITY_NONE", 0), ("INTENSITY_F32", 1), ("INTENSITY_U8", 2)):
        assert re.search(r"LOCGPU_%s = %d\b" % (name, value), block), name
        assert getattr(api, name) == value
    body = re.search(r"typedef struct locgpu_point_layout \{(.*?)\} locgpu_point_layout;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in api.PointLayoutC._fields_], fields
    assert ctypes.sizeof(api.PointLayoutC) == 48 and api.PointLayoutC.time_scale.offset == 40 and api.PointLayoutC.min_range.offset == 32


def test_point_layout_marshals_field_for_field(api):
    for name, attr in cases.READY.items():
        assert getattr(api, attr) == cases.LAYOUTS[name], name  # plain data, the tests' own tables
    L = api.point_layout(api.LAYOUT_OUSTER)
    assert (L.stride_bytes, L.xyz_offset, L.time_offset, L.time_kind, L.ring_offset, L.ring_kind, L.intensity_offset, L.intensity_kind) == \
        (48, 0, 20, api.TIME_U32, 26, api.RING_U8, 16, api.INTENSITY_F32)
    assert L.min_range == 4.0 and L.reserved == 0 and L.time_scale == 1e-9
    V = api.point_layout(api.LAYOUT_VELODYNE_PACKED, min_range=0.5)
    assert (V.stride_bytes, V.time_offset, V.time_kind, V.ring_offset, V.ring_kind, V.intensity_offset, V.min_range, V.time_scale) == \
        (22, 18, api.TIME_F32, 16, api.RING_U16, 12, 0.5, 1.0)
    assert api.point_layout(V, stride_bytes=24).stride_bytes == 24 and api.point_layout(V).min_range == 0.5
    raw = bytes(L)
    assert np.frombuffer(raw[:32], "<u4").tolist() == [48, 0, 20, 3, 26, 1, 16, 1]
    assert np.frombuffer(raw[32:36], "<f4")[0] == 4.0 and np.frombuffer(raw[40:48], "<f8")[0] == 1e-9
    with pytest.raises(TypeError):
        api.point_layout(api.LAYOUT_VELODYNE, colour=3)


def test_refusals_without_a_device(api):
    L = api.lib()
    fake = ctypes.c_void_p(64)  # never dereferenced: the argument checks come first, then the NULL handle
    n = ctypes.c_size_t(7)

    def text(rc):
        assert rc == INVALID
        t = L.locgpu_last_error(None)
        assert t and len(t) > 10
        return t

    def all_four(layout, word, deskew_only=False):
        p = ctypes.byref(layout) if layout is not None else None
        calls = [("batch_upload_records_deskew", lambda: L.locgpu_batch_upload_records_deskew(None, p, fake, fake, fake, fake, None, None)),
                 ("cloud_upload_records_deskew", lambda: L.locgpu_cloud_upload_records_deskew(None, p, fake, 5, 0.0, fake, None, ctypes.byref(n)))]
        if not deskew_only:
            calls += [("batch_upload_records", lambda: L.locgpu_batch_upload_records(None, p, fake, fake, None)),
                      ("cloud_upload_records", lambda: L.locgpu_cloud_upload_records(None, p, fake, 5, None, ctypes.byref(n)))]
        for who, call in calls:
            t = text(call())
            assert who.encode() in t and word.encode() in t, (who, word, t)

    good = api.LAYOUT_RSLIDAR
    all_four(None, "layout is NULL")
    all_four(api.point_layout(good), "NULL")  # a good layout: the NULL handle is what is refused
    for stride in (0, 11, 65, 2 ** 32 - 1):
        all_four(api.point_layout(good, stride_bytes=stride), "stride_bytes")
    # offset + size > stride, without overflow
    all_four(api.point_layout(good, xyz_offset=21), "xyz field does not fit")
    all_four(api.point_layout(good, xyz_offset=2 ** 32 - 4), "xyz field does not fit")
    all_four(api.point_layout(good, time_offset=25), "time field does not fit")
    all_four(api.point_layout(good, time_offset=2 ** 32 - 1), "time field does not fit")
    all_four(api.point_layout(good, ring_offset=31), "ring field does not fit")
    all_four(api.point_layout(good, intensity_offset=29), "intensity field does not fit")
    all_four(api.point_layout(good, intensity_offset=31, intensity_kind=api.INTENSITY_U8), "NULL")  # a byte at the last offset fits
    # fields that overlap xyz
    all_four(api.point_layout(good, ring_offset=11), "ring field overlaps xyz")
    all_four(api.point_layout(good, xyz_offset=8, intensity_offset=4), "NULL")  # intensity ends where xyz begins
    all_four(api.point_layout(good, xyz_offset=8, intensity_offset=5), "intensity field overlaps xyz")
    all_four(api.point_layout(good, xyz_offset=12, time_offset=5), "time field overlaps xyz")
    # unknown kinds
    all_four(api.point_layout(good, time_kind=4), "time_kind")
    all_four(api.point_layout(good, ring_kind=3), "ring_kind")
    all_four(api.point_layout(good, intensity_kind=3), "intensity_kind")
    # no time field: the deskewed calls only
    all_four(api.point_layout(good, time_kind=api.TIME_NONE), "LOCGPU_TIME_NONE", deskew_only=True)
    assert b"NULL" in text(L.locgpu_batch_upload_records(None, ctypes.byref(api.point_layout(good, time_kind=api.TIME_NONE)), fake, fake, None))
    # min_range and time_scale
    for bad in (-1.0, float("nan"), float("inf")):
        all_four(api.point_layout(good, min_range=bad), "min_range")
    for bad in (0.0, float("nan"), float("-inf")):
        all_four(api.point_layout(good, time_scale=bad), "time_scale")
    all_four(api.point_layout(good, min_range=0.0, time_scale=-1e-9), "NULL")  # both allowed
    # the tools' entry points
    assert b"records_deskew_debug" in text(L.locgpu_records_deskew_debug(None, 1))
    assert b"records_deskew_matrices" in text(L.locgpu_records_deskew_matrices(None, 0, None, 0, ctypes.byref(n)))
    assert b"records_ingest_times" in text(L.locgpu_records_ingest_times(None, None))
    assert n.value == 7
