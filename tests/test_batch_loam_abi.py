"""LOAM on whole batches, host side: the header, the library and the Python binding agree on locgpu_batch_loam_extract and
locgpu_loam_align_batches, the header cites the reference lines it restates and keeps the LoamRegistration block's limits true, and the
NULL-argument refusals come back as LOCGPU_ERR_INVALID before any device is touched (so they need no GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_batch_loam_extract", "locgpu_loam_align_batches")
INVALID = -1  # LOCGPU_ERR_INVALID


def _declaration(header, name):
    m = re.search(r"LOCGPU_API\s+int\s+%s\s*\(" % name, header)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(header[i], 0)
        i += 1
    return re.sub(r"/\*.*?\*/", "", header[m.end():i - 1], flags=re.S)


def test_names_are_exported_declared_and_bound_with_the_headers_argument_counts(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        n_args = len(_declaration(header, name).split(","))
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert hasattr(L, name) and name in api.ABI_SYMBOLS, name
        assert len(getattr(L, name).argtypes) == n_args, (name, n_args)
    assert len(_declaration(header, "locgpu_batch_loam_extract").split(",")) == 8
    assert len(_declaration(header, "locgpu_loam_align_batches").split(",")) == 6
    assert callable(api.Batch.loam_extract) and callable(api.Loam.align_batches)
    # locgpu_batch_loam_extract stands next to the single-cloud picker, locgpu_loam_align_batches in the resident part
    assert header.index("locgpu_cloud_loam_extract(") < header.index("locgpu_batch_loam_extract(") < header.index("locgpu_loam_set_target_cloud(")
    assert header.index("locgpu_batch_preprocess(") < header.index("locgpu_loam_align_batches(")


def test_header_keeps_the_pinned_limits_and_cites_the_reference():
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    limits = header[header.index("---- LoamRegistration"):header.index("locgpu_loam_opts_default")]
    assert "no batched resident form of n DIFFERENT scans" in limits and "no batched resident form" in limits
    assert "locgpu_loam_align_batches" in limits  # ... and the sentence around the phrase says where that form is
    block = header[header.index("---- LOAM on a whole BATCH"):header.index("locgpu_loam_align_batches(")]
    for cite in ("loam_feature_extract.cpp:19-151", "lio.cpp:323", "lio.cpp:485-486", "65535", "131", "6 x 2048"):
        assert cite in block, cite


def test_null_arguments_are_refused_without_a_device(api):
    L = api.lib()
    fake = ctypes.c_void_p(64)  # never dereferenced: the NULL arguments are tested first
    counts = np.full(3, 7, np.int32)
    poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64), (2, 1))
    out = np.full((2, 7), 3.0)
    assert L.locgpu_batch_loam_extract(None, None, 16, None, None, None, None, None) == INVALID
    assert L.locgpu_batch_loam_extract(None, fake, 16, None, None, counts.ctypes.data, counts.ctypes.data, counts.ctypes.data) == INVALID
    assert L.locgpu_last_error(None)
    assert (counts == 7).all()
    assert L.locgpu_loam_align_batches(None, fake, fake, poses.ctypes.data, out.ctypes.data, None) == INVALID
    assert L.locgpu_loam_align_batches(None, None, None, None, None, None) == INVALID
    assert (out == 3.0).all()
