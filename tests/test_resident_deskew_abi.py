"""The deskew of a resident batch on the host side: its entry points are exported by liblocgpu.so, declared in include/locgpu.h with
the reference lines they relate to and bound in loc_lib_amd/api.py with the header's argument counts; the older blocks no longer list
it as out of scope; the refusals that need neither a handle nor a device come back as LOCGPU_ERR_INVALID with a text."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_batch_keep_times", "locgpu_batch_download_times", "locgpu_batch_deskew", "locgpu_batch_deskew_times", "locgpu_motion_from_poses")
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
    for name in ("locgpu_batch_deskew", "locgpu_motion_from_poses"):
        above = header[:header.index("LOCGPU_API int %s(" % name)]
        assert "loc.cpp:232" in above[above.rindex("/*"):], name
    for cls, method in ((api.Batch, "keep_times"), (api.Batch, "download_times"), (api.Batch, "deskew"), (api.Context, "batch_deskew_times")):
        assert callable(getattr(cls, method))
    assert callable(api.motion_from_poses)
    # the block stands directly behind the point-record block and carries the definition
    start = header.index("---- Deskew of a resident batch")
    assert header.index("locgpu_records_ingest_times(") < start < header.index("locgpu_submap_create(")
    block = header[start:header.index("LOCGPU_API int locgpu_batch_keep_times(")]
    for word in ("loc.cpp:232", "lio.cpp:465", "math_utils.h:470-517", "off by default", "time_offsets == NULL", "nothing is added", "SAME device function",
                 "in place", "exactly as it was", "0.5", "no atomics", "never holds times", "no resident times", "Out of scope", "locgpu_cloud_*"):
        assert word in block, word
    spelled = header[header.index("The motion of n consecutive scans"):header.index("locgpu_motion_from_poses(const")]
    for word in ("((aw bw - ax bx) - ay by) - az bz", "(R[r][0] v0 + R[r][1] v1) + R[r][2] v2", "(-x, -y, -z, w)", "t1 + R(q1) t2", "2.0 * t[n-1] - t[n-2]", "2.0 * t[0] - t[1]",
                 "nothing normalised", "n < 2"):
        assert word in spelled, word
    # the two older blocks no longer leave it out for the batch forms
    for title in ("---- Range-image ingest, motion-compensated", "---- Point-record ingest"):
        older = header[header.index(title):]
        older = older[:older.index("*/")]
        assert "re-compensating a batch that is already decoded" not in older and "previous two poses" not in older
        assert "Deskew of a resident batch" in older[older.index("Out of scope"):]


def test_refusals_without_a_device(api):
    L = api.lib()
    fake = ctypes.c_void_p(64)  # never dereferenced: the NULL handle is refused first
    n = ctypes.c_size_t(7)

    def text(rc):
        assert rc == INVALID
        t = L.locgpu_last_error(None)
        assert t and len(t) > 10
        return t

    assert b"batch_keep_times" in text(L.locgpu_batch_keep_times(None, 1))
    assert b"batch_download_times" in text(L.locgpu_batch_download_times(None, 0, None, 0, ctypes.byref(n)))
    assert b"batch_deskew: NULL batch" in text(L.locgpu_batch_deskew(None, None, None, fake, None))
    assert b"batch_deskew_times" in text(L.locgpu_batch_deskew_times(None, None))
    assert b"motion_from_poses" in text(L.locgpu_motion_from_poses(None, None, 5, None, None))
    assert n.value == 7
