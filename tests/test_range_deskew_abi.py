"""The motion-compensated range-image ingest on the host side: its entry points are exported by liblocgpu.so, declared in
include/locgpu.h and bound in loc_lib_amd/api.py with the header's argument counts; each comment cites math::PoseInterp and
CloudConver::Conver; the refusals that need no device come back as LOCGPU_ERR_INVALID with a text."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_sensor_set_col_times", "locgpu_batch_upload_ranges_deskew", "locgpu_cloud_upload_ranges_deskew", "locgpu_range_deskew_matrices",
         "locgpu_range_deskew_times")
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
        for cite in ("math_utils.h:470-517", "cloud_subscriber.cpp:7-29"):
            assert cite in comment, (name, cite)
    for cls, method in ((api.Sensor, "set_col_times"), (api.Batch, "upload_ranges_deskew"), (api.Cloud, "upload_ranges_deskew"),
                        (api.Context, "range_deskew_matrices"), (api.Context, "range_deskew_times")):
        assert callable(getattr(cls, method))
    # the new block stands directly behind the range-image block and says what it leaves out
    start = header.index("---- Range-image ingest, motion-compensated")
    assert header.index("locgpu_range_ingest_times(") < start < header.index("locgpu_submap_create(")
    block = header[start:header.index("locgpu_sensor_set_col_times(")]
    for word in ("byte for byte", "exactly as it was", "Out of scope", "per-point time fields", "not normalised", "1e-6", "DBL_EPSILON", "0.5 s",
                 "summed left to right", "NOT the identity"):
        assert word in block, word
    # the struct the binding hands over is the header's: same fields in the same order
    body = re.search(r"typedef struct locgpu_sweep_motion \{(.*?)\} locgpu_sweep_motion;", header, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(None, 1)[1] if not decl.startswith("const") else decl.split("*", 1)[1]
        fields += [n.strip() for n in names.split(",")]
    assert fields == [f[0] for f in api.SweepMotionC._fields_], fields
    assert ctypes.sizeof(api.SweepMotionC) == 8 + 3 * ctypes.sizeof(ctypes.c_void_p)


def test_refusals_without_a_device(api):
    L = api.lib()
    fake = ctypes.c_void_p(64)  # never dereferenced: the NULL refusal comes first
    n = ctypes.c_size_t(7)

    def refused(rc):
        assert rc == INVALID
        text = L.locgpu_last_error(None)
        assert text and len(text) > 10
        return text

    assert b"sensor_set_col_times" in refused(L.locgpu_sensor_set_col_times(None, fake))
    assert b"batch_upload_ranges_deskew" in refused(L.locgpu_batch_upload_ranges_deskew(None, fake, fake, fake, None))
    assert b"cloud_upload_ranges_deskew" in refused(L.locgpu_cloud_upload_ranges_deskew(None, fake, fake, fake, None, ctypes.byref(n)))
    assert b"range_deskew_matrices" in refused(L.locgpu_range_deskew_matrices(None, 0, None, 0, ctypes.byref(n)))
    assert b"range_deskew_times" in refused(L.locgpu_range_deskew_times(None, None))
    assert n.value == 7


def test_sweep_motion_marshalling(api):
    import numpy as np
    import pytest
    m, keep = api.sweep_motion(2, np.zeros((2, 5)), np.zeros((2, 5, 7)), [0.0, 1.0])
    assert m.n_knots == 5 and m.reserved == 0 and m.knot_times == keep[0].ctypes.data and m.knot_poses == keep[1].ctypes.data and m.ref_times == keep[2].ctypes.data
    with pytest.raises(ValueError):
        api.sweep_motion(2, np.zeros((2, 5)), np.zeros((2, 4, 7)), [0.0, 1.0])
    with pytest.raises(ValueError):
        api.sweep_motion(2, np.zeros((2, 5)), np.zeros((2, 5, 7)), [0.0])
