"""The LOAM matcher's score and search on the host side: the header, the library and the Python binding agree on the names, and the
argument-only refusals of locgpu_loam_create_on come back as LOCGPU_ERR_INVALID before any device is touched (so they need no GPU);
the façade's GetFitnessScore keeps the reference's stub without the opt-in and reports +infinity before the first ScanMatch with it."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the five new entry points, and the per-class score that was there before them
NAMES = ("locgpu_loam_fitness", "locgpu_loam_fitness_cloud", "locgpu_loam_init_search", "locgpu_loam_init_search_cloud", "locgpu_loam_create_on",
         "locgpu_loam_fitness_resident")
INVALID = -1  # LOCGPU_ERR_INVALID


def test_header_library_and_binding_agree_on_the_names(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"LOCGPU_API\s+[\w\s\*]+?\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in api.ABI_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    for method in ("on", "fitness", "fitness_cloud", "init_search", "init_search_cloud"):
        assert callable(getattr(api.Loam, method))
    # the header defines the joint score and says what is and is not available
    block = header[header.index("---- The JOINT score"):header.index("locgpu_loam_init_search(")]
    for word in ("POOLED", "loam_registration.cpp:76-79", "un-rounded", "[3i] joint", "at most 256"):
        assert word in block, word
    limits = header[header.index("---- LoamRegistration"):header.index("locgpu_loam_opts_default")]
    assert "SHARED-SOURCE" in limits and "no batched resident form of n DIFFERENT scans" in limits


def test_create_on_refuses_by_argument_without_a_device(api):
    L = api.lib()
    h = ctypes.c_void_p(5)
    fake = ctypes.c_void_p(64)  # never dereferenced: every refusal below comes first
    opts = api.loam_opts()
    assert L.locgpu_loam_create_on(None, None, ctypes.byref(opts), ctypes.byref(h)) == INVALID
    assert h.value is None and L.locgpu_loam_last_error(None)
    assert L.locgpu_loam_create_on(fake, None, ctypes.byref(opts), ctypes.byref(h)) == INVALID  # the edge class is on and has no context
    assert L.locgpu_loam_create_on(None, fake, ctypes.byref(opts), ctypes.byref(h)) == INVALID
    assert L.locgpu_loam_create_on(fake, fake, None, ctypes.byref(h)) == INVALID
    assert L.locgpu_loam_create_on(fake, fake, ctypes.byref(opts), None) == INVALID
    assert L.locgpu_loam_create_on(fake, fake, ctypes.byref(opts), ctypes.byref(h)) == INVALID  # one context given twice
    for bad in (api.loam_opts(use_surf_points=0, use_edge_points=0), api.loam_opts(surf=api.icp_opts(method=api.P2PLANE_MAP)), api.loam_opts(edge=api.icp_opts(method=9))):
        assert L.locgpu_loam_create_on(fake, fake, ctypes.byref(bad), ctypes.byref(h)) == INVALID
        assert h.value is None
    # NULL handles of the new calls
    assert L.locgpu_loam_fitness(None, None, 0, None, 0, 12, None, 1, 1.0, None) == INVALID
    assert L.locgpu_loam_fitness_cloud(None, None, None, None, 1, 1.0, None) == INVALID
    assert L.locgpu_loam_init_search(None, None, 0, None, 0, 12, None, 1, None, None, None, None, None) == INVALID
    assert L.locgpu_loam_init_search_cloud(None, None, None, None, 1, None, None, None, None, None) == INVALID


def test_facade_keeps_the_stub_and_reports_infinity_before_a_scan_match():
    """tests/cpp/facade_loam_search without arguments: GetFitnessScore() is 0.0f without EnableFitnessScore, +infinity (and a reason
    in LastError) before the first ScanMatch with it, and InitialPoseSearch without targets is refused — no device is touched.
    The driver is a build product under tests/: made here when it is absent or stale (as test_abi_and_host.py does with
    facade_scanmatch), so the test does not depend on tests/cpp being left as build() left it."""
    exe = os.path.join(ROOT, "tests", "cpp", "facade_loam_search")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "loc_lib_amd", "host"), "../../tests/cpp/facade_loam_search"], stdout=subprocess.DEVNULL)
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
