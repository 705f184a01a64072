"""The global map on the host side: locgpu_clouds_merge, locgpu_batch_merge and locgpu_batch_export_cloud are exported by liblocgpu.so,
declared in include/locgpu.h and bound in loc_lib_amd/api.py with the header's argument counts; the header block says where the
reference does it; the refusals that need no device (NULL handles) come back as LOCGPU_ERR_INVALID with a text and leave their
outputs alone."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_clouds_merge", "locgpu_batch_merge", "locgpu_batch_export_cloud")
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
    assert callable(api.Context.clouds_merge) and callable(api.Batch.merge) and callable(api.Batch.export_cloud)
    # one new block at the end of the header, behind locgpu_loam_submap_info, that cites the reference
    start = header.index("---- The global map")
    assert start > header.index("locgpu_loam_submap_info(")
    block = header[start:header.index("locgpu_batch_export_cloud(")]
    for word in ("lio.cpp:550-614", ":131-207", ":254", ":275", ":571", "voxel_filter.cpp:19-25", "byte for byte", "intensity is 0",
                 "leaf == 0", "poses == NULL", "exactly as it was"):
        assert word in block, word
    for name in NAMES:
        assert header.index(name + "(") > start, name


def test_null_handles_are_refused_without_a_device(api):
    L = api.lib()
    fake = ctypes.c_void_p(64)  # never dereferenced: the NULL refusals come first
    passthrough = ctypes.c_int(7)
    list1 = (ctypes.c_void_p * 1)(None)
    pt = ctypes.byref(passthrough)
    for ctx, clouds, out in ((None, list1, fake), (None, None, fake), (None, list1, None)):
        assert L.locgpu_clouds_merge(ctx, clouds, None, 1, 0.5, out, pt) == INVALID
        assert b"clouds_merge" in L.locgpu_last_error(None)
    assert L.locgpu_batch_merge(None, None, None, 0.5, fake, pt) == INVALID
    assert b"batch_merge" in L.locgpu_last_error(None)
    assert L.locgpu_batch_merge(None, None, None, 0.5, None, pt) == INVALID
    assert L.locgpu_batch_export_cloud(None, 0, fake) == INVALID
    assert b"batch_export_cloud" in L.locgpu_last_error(None)
    assert L.locgpu_batch_export_cloud(None, 0, None) == INVALID
    assert passthrough.value == 7
