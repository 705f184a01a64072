"""The resident LOAM entry points on the host side: the header, the library and the Python binding agree on the new names, the header
cites the reference lines it restates, and the argument-only refusals come back as LOCGPU_ERR_INVALID before any device is touched."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_loam_set_target_cloud", "locgpu_loam_set_target_cloud_async", "locgpu_loam_scan_match_cloud", "locgpu_loam_fitness_resident",
         "locgpu_loam_submap_create", "locgpu_loam_submap_destroy", "locgpu_loam_submap_add_keyframe", "locgpu_loam_submap_clouds",
         "locgpu_loam_submap_info")
INVALID = -1  # LOCGPU_ERR_INVALID


def test_header_library_and_binding_agree_on_the_resident_loam_names(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    for name in NAMES:
        assert re.search(r"LOCGPU_API\s+[\w\s\*]+?\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in api.ABI_SYMBOLS, name
    for method in ("set_target_cloud", "scan_match_cloud", "fitness_resident"):
        assert callable(getattr(api.Loam, method))
    for method in ("add_keyframe", "clouds", "close"):
        assert callable(getattr(api.LoamSubmap, method))
    # the matcher's entry points cite loam_registration.cpp, the pair of maps cites lio.cpp and restates the two details
    for name in ("locgpu_loam_set_target_cloud", "locgpu_loam_set_target_cloud_async", "locgpu_loam_scan_match_cloud", "locgpu_loam_fitness_resident"):
        pos = header.index(name + "(")
        assert re.search(r"loam_registration\.cpp:\d+", header[max(0, pos - 1400):pos]), name
    pos = header.index("locgpu_loam_submap_create(")
    block = header[header.index("The PAIR of local maps"):pos]
    for cite in ("lio.cpp:331-409", ":338-339", ":348-349", ":346", ":485-486", ":382-388", ":343-344", ":379-380", "UNFILTERED"):
        assert cite in block, cite
    limits = header[header.index("---- LoamRegistration"):header.index("locgpu_loam_opts_default")]
    for limit in ("hipGraph", "sharded", "pools", "map planes", "no batched resident form"):
        assert limit in limits, limit


def test_argument_only_refusals_need_no_device(api):
    L = api.lib()
    pose = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    out = np.full(7, 3.0)
    fit = (api.Fitness * 2)()
    st = api.AlignStats()
    fake = ctypes.c_void_p(64)  # never dereferenced: the handle is tested first
    h = ctypes.c_void_p(5)
    # NULL handles
    assert L.locgpu_loam_set_target_cloud(None, fake, fake) == INVALID
    assert L.locgpu_loam_set_target_cloud_async(None, fake, fake) == INVALID
    assert L.locgpu_loam_scan_match_cloud(None, fake, fake, pose.ctypes.data, out.ctypes.data, ctypes.byref(st), None) == INVALID
    assert L.locgpu_loam_fitness_resident(None, pose.ctypes.data, 1.0, fit) == INVALID
    assert (out == 3.0).all()
    assert L.locgpu_loam_submap_add_keyframe(None, fake, fake, pose.ctypes.data) == INVALID
    assert L.locgpu_loam_submap_info(None, None, None, None) == INVALID
    assert L.locgpu_loam_submap_clouds(None, ctypes.byref(h), ctypes.byref(h)) == INVALID
    L.locgpu_loam_submap_destroy(None)
    # NULL context / NULL output of the create
    assert L.locgpu_loam_submap_create(None, 2, 0.5, ctypes.byref(h)) == INVALID
    assert L.locgpu_loam_submap_create(fake, 2, 0.5, None) == INVALID
