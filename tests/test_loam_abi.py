"""The LOAM matcher's C ABI on the host side: the header, the library and the Python binding agree on the new names, the defaults are
LoamOption's, and the argument-only refusals come back as LOCGPU_ERR_INVALID before any device is touched (so they need no GPU)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locgpu_loam_opts_default", "locgpu_loam_create", "locgpu_loam_destroy", "locgpu_loam_last_error", "locgpu_loam_set_target", "locgpu_loam_hb",
         "locgpu_loam_scan_match", "locgpu_loam_align_batch")
INVALID = -1  # LOCGPU_ERR_INVALID


def test_header_library_and_binding_agree_on_the_loam_names(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    for name in NAMES:
        assert re.search(r"LOCGPU_API\s+[\w\s\*]+?\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in api.ABI_SYMBOLS, name
    for method in ("set_target", "hb", "scan_match", "align_batch"):
        assert callable(getattr(api.Loam, method))
    # every entry point cites the reference lines it replaces, and the header states the limits
    for name in ("locgpu_loam_set_target", "locgpu_loam_hb", "locgpu_loam_scan_match", "locgpu_loam_align_batch"):
        pos = header.index(name + "(")
        assert re.search(r"loam_registration\.cpp:\d+", header[max(0, pos - 1400):pos]), name
    block = header[header.index("---- LoamRegistration"):header.index("locgpu_loam_opts_default")]
    for limit in ("EAGER", "sharded", "pools", "LOCGPU_P2PLANE_MAP"):
        assert limit in block, limit
    assert "3 the SURFACE" in header and "4 the EDGE" in header  # the new status values, in the struct's comment


def test_defaults_are_loam_options_defaults(api):
    o = api.loam_opts()  # LoamOption, loam_registration.hpp:22-36
    assert (o.surf.method, o.edge.method) == (api.P2PLANE, api.P2LINE)
    assert (o.max_iteration, o.eps, o.use_surf_points, o.use_edge_points) == (20, 1e-3, 1, 1)
    assert (o.surf.max_plane_distance, o.edge.max_line_distance, o.surf.min_effective_pts, o.edge.min_effective_pts) == (0.1, 0.5, 10, 10)
    assert ctypes.sizeof(api.LoamOpts) == 2 * ctypes.sizeof(api.IcpOpts) + 24


def test_argument_only_refusals_need_no_device(api):
    L = api.lib()
    pose = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    out = np.full(7, 3.0)
    pts = np.zeros((4, 3), np.float32)
    H, B = np.zeros(36), np.zeros(6)
    st = api.AlignStats()
    ptrs = (ctypes.c_void_p * 1)(pts.ctypes.data)
    cnts = (ctypes.c_size_t * 1)(4)
    # NULL handles
    assert L.locgpu_loam_set_target(None, pts.ctypes.data, 4, pts.ctypes.data, 4, 12) == INVALID
    assert L.locgpu_loam_hb(None, pts.ctypes.data, 4, pts.ctypes.data, 4, 12, pose.ctypes.data, H.ctypes.data, B.ctypes.data, None, None) == INVALID
    assert L.locgpu_loam_scan_match(None, pts.ctypes.data, 4, pts.ctypes.data, 4, 12, pose.ctypes.data, out.ctypes.data, ctypes.byref(st), None, 0) == INVALID
    assert L.locgpu_loam_align_batch(None, 1, ptrs, cnts, ptrs, cnts, 12, pose.ctypes.data, out.ctypes.data, None) == INVALID
    assert (out == 3.0).all()
    L.locgpu_loam_destroy(None)
    # options refused before a device is asked for: the map-plane fast mode, an unknown method, nothing switched on, no options at all
    h = ctypes.c_void_p(5)
    for bad in (api.loam_opts(surf=api.icp_opts(method=api.P2PLANE_MAP)), api.loam_opts(edge=api.icp_opts(method=api.P2PLANE_MAP)),
                api.loam_opts(edge=api.icp_opts(method=9)), api.loam_opts(use_surf_points=0, use_edge_points=0)):
        assert L.locgpu_loam_create(0, ctypes.byref(bad), ctypes.byref(h)) == INVALID
        assert h.value is None and L.locgpu_loam_last_error(None)
    assert L.locgpu_loam_create(0, None, ctypes.byref(h)) == INVALID
    assert L.locgpu_loam_create(0, ctypes.byref(api.loam_opts()), None) == INVALID
    # a switched-off class may carry any method: it is never read
    ok = api.loam_opts(use_edge_points=0, edge=api.icp_opts(method=api.P2PLANE_MAP))
    assert L.locgpu_loam_create(0, ctypes.byref(ok), ctypes.byref(h)) in (0, -2)  # a handle with a GPU, LOCGPU_ERR_NO_DEVICE without one
    if h.value:
        L.locgpu_loam_destroy(h)
