"""The range-image ingest on the host side: its entry points are exported by liblocgpu.so, declared in include/locgpu.h and bound in
loc_lib_amd/api.py with the header's argument counts; the header says what is computed and where the reference does it; the refusals
that need no device come back as LOCGPU_ERR_INVALID with a text."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_sensor_create", "locgpu_batch_upload_ranges", "locgpu_batch_download_rings", "locgpu_batch_loam_extract_resident",
         "locgpu_cloud_upload_ranges", "locgpu_range_ingest_times")
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
        # every entry point cites the reference function it stands for, in the comment right above it
        above = header[:m.start()]
        comment = above[above.rindex("/*"):]
        for cite in ("cloud_subscriber.cpp:7-29", "point_cloud_utils.h:41-44"):
            assert cite in comment, (name, cite)
    assert re.search(r"LOCGPU_API\s+void\s+locgpu_sensor_destroy\s*\(\s*locgpu_sensor\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"\bT locgpu_sensor_destroy$", exported, re.M) and "locgpu_sensor_destroy" in api.ABI_SYMBOLS
    assert len(L.locgpu_sensor_destroy.argtypes) == 1
    for cls, method in ((api.Batch, "upload_ranges"), (api.Batch, "download_rings"), (api.Batch, "loam_extract_resident"), (api.Cloud, "upload_ranges")):
        assert callable(getattr(cls, method))
    assert callable(api.Sensor) and callable(api.SensorModel)
    block = header[header.index("---- Range-image ingest"):header.index("locgpu_cloud_upload_ranges(")]
    for word in ("byte for byte", "exactly as it was", "Out of scope", "no atomics"):
        assert word in block, word
    # the struct the binding hands over is the header's: same fields in the same order
    body = re.search(r"typedef struct locgpu_sensor_model \{(.*?)\} locgpu_sensor_model;", header, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(None, 1)[1] if not decl.startswith("const") else decl.split("*", 1)[1]
        fields += [n.strip() for n in names.split(",")]
    assert fields == [f[0] for f in api.SensorModelC._fields_], fields


def test_synth_range_image_needs_no_device(api, synth):
    m = api.SensorModel(16, 90, 0.004, 4.0, *synth.sensor_tables(16, 90))
    img = synth.make_range_image(3, m)
    assert img.shape == (16, 90) and img.dtype == np.uint16 and (img > 0).sum() > 16 * 90 // 2
    assert np.array_equal(img, synth.make_range_image(3, m))
    # the generator's 4 m cut is in the image as it is in the cloud: every return decodes to 4 m or more, within half a count
    assert int(img[img > 0].min()) >= int(round((4.0 - 0.002) / 0.004))


def test_refusals_without_a_device(api):
    L = api.lib()
    fake = ctypes.c_void_p(64)  # never dereferenced: the NULL refusal comes first
    n = ctypes.c_size_t(7)
    out = ctypes.c_void_p()
    assert L.locgpu_sensor_create(None, fake, ctypes.byref(out)) == INVALID
    assert L.locgpu_last_error(None)
    assert L.locgpu_batch_upload_ranges(None, fake, fake, None) == INVALID
    assert L.locgpu_batch_download_rings(None, 0, None, 0, ctypes.byref(n)) == INVALID
    assert L.locgpu_batch_loam_extract_resident(None, 16, None, None, None, None, None) == INVALID
    assert L.locgpu_cloud_upload_ranges(None, fake, fake, None, ctypes.byref(n)) == INVALID
    assert L.locgpu_range_ingest_times(None, None) == INVALID
    L.locgpu_sensor_destroy(None)
