"""The batch front-end on the host side: locgpu_batch_preprocess, locgpu_batch_upload_clouds and locgpu_batch_download_scan are exported
by liblocgpu.so, declared in include/locgpu.h and bound in loc_lib_amd/api.py with the header's argument counts; the refusals that need
no device (NULL batches) come back as LOCGPU_ERR_INVALID."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_batch_preprocess", "locgpu_batch_upload_clouds", "locgpu_batch_download_scan")
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
    for method in ("preprocess", "upload_clouds", "download_scan"):
        assert callable(getattr(api.Batch, method))
    # the header says what the pass computes and where the reference does it
    block = header[header.index("---- The front-end on a whole BATCH"):header.index("locgpu_batch_download_scan(")]
    for word in ("loc.cpp:217-218", "lio.cpp:236", "voxel_filter.cpp:19-25", "point_cloud_utils.h:13-20", "byte for byte", "dst == src", "is exactly as it was"):
        assert word in block, word


def test_null_batches_are_refused_without_a_device(api):
    L = api.lib()
    fake = ctypes.c_void_p(64)  # never dereferenced: the NULL refusal comes first
    n = ctypes.c_size_t(7)
    assert L.locgpu_batch_preprocess(None, 1.0, None, None, None) == INVALID
    assert L.locgpu_last_error(None)
    assert L.locgpu_batch_upload_clouds(None, fake, 1) == INVALID
    assert L.locgpu_batch_download_scan(None, 0, None, 0, 16, ctypes.byref(n)) == INVALID
