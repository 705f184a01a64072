"""Pairwise batch ICP on the host side: the forest and pairs entry points are exported by liblocgpu.so, declared in include/locgpu.h
with the reference lines they relate to and bound in loc_lib_amd/api.py with the header's argument counts; a NULL context is refused
without a device; and the host packing of a forest (csrc/kdtree_build.cpp, build_packed_forest) passes its stand-alone harness,
tests/cpp/forest_pack_check.cpp, with and without AddressSanitizer + UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loc_lib_amd", "csrc")
# name → the reference lines its own comment must cite
NAMES = {
    "locgpu_icp_set_target_forest": ("icp_registration.cpp:9-29", "test_node.cpp:256-315"),
    "locgpu_icp_set_target_forest_batch": ("icp_registration.cpp:9-29", "test_node.cpp:256-315"),
    "locgpu_icp_forest_info": ("icp_registration.cpp:9-29",),
    "locgpu_icp_align_pairs": ("icp_registration.cpp:216-244", "test_node.cpp:256-315", ":437-460", "test_node.cpp:289"),
    "locgpu_icp_fitness_pairs": ("icp_registration.cpp:216-244", "test_node.cpp:256-315"),
}
INVALID = -1  # LOCGPU_ERR_INVALID


def test_header_library_and_binding_agree(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, cites in NAMES.items():
        m = re.search(r"LOCGPU_API\s+int\s+%s\s*\(([^;]*)\);" % name, header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert hasattr(L, name) and name in api.ABI_SYMBOLS, name
        assert len(getattr(L, name).argtypes) == len(args.split(",")), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        above = header[:m.start()]
        comment = above[above.rindex("/*"):]
        for cite in cites:
            assert cite in comment, (name, cite)
    for method in ("icp_set_target_forest", "icp_set_target_forest_batch", "icp_forest_info", "icp_align_pairs", "icp_fitness_pairs"):
        assert callable(getattr(api.Context, method)), method
    # the block says what a forest is, what it may hold, which calls a forest context answers and what is left out
    start = header.index("---- Pairwise batch ICP")
    block = header[start:header.index("LOCGPU_API int locgpu_icp_set_target_forest(")]
    for word in ("test_node.cpp:256-315", ":437-460", "icp_registration.cpp:9-29", "icp_registration.cpp:216-244", "2^29 slots", "exactly as it was",
                 "locgpu_knn", "locgpu_icp_align*", "locgpu_icp_hb*", "locgpu_icp_scan_match", "locgpu_icp_fitness*", "locgpu_icp_init_search", "locgpu_pool_*",
                 "map planes", "grid search", "locgpu_loam_create_on", "ordinary again", "Not covered", "NDT and LOAM pairs", "scan pools", "hipGraph", "sharded",
                 "facade", "bench.py", "asynchronous"):
        assert word in block, word
    # the status of a scan that was given no target is a constant of its own, named in the stats struct's comment too
    m = re.search(r"#define\s+LOCGPU_STATUS_NO_PAIR_TARGET\s+(\d+)", header)
    assert m and int(m.group(1)) == api.STATUS_NO_PAIR_TARGET == 5
    stats = header[header.index("typedef struct locgpu_align_stats"):header.index("} locgpu_align_stats;")]
    assert "LOCGPU_STATUS_NO_PAIR_TARGET" in stats
    for other in re.findall(r"\b(\d) (?:direct-NDT|incremental NDT|the SURFACE|the EDGE)", stats):
        assert int(other) != api.STATUS_NO_PAIR_TARGET


def test_null_context_is_refused_without_a_device(api):
    L = api.lib()
    assert L.locgpu_icp_set_target_forest(None, None, None, 1, 16) == INVALID
    assert L.locgpu_icp_set_target_forest_batch(None, None) == INVALID
    assert L.locgpu_icp_forest_info(None, None, None, None) == INVALID
    assert L.locgpu_icp_align_pairs(None, None, None, None, None, None, None) == INVALID
    assert L.locgpu_icp_fitness_pairs(None, None, None, None, 1.0, None) == INVALID


def _harness(tmp_path, tag, flags):
    exe = str(tmp_path / ("forest_pack_" + tag))
    cmd = ["g++", "-std=c++17"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "forest_pack_check.cpp"), os.path.join(CSRC, "kdtree_build.cpp"), "-o", exe,
                                           "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return exe, r


def test_forest_packing_harness(tmp_path):
    """Three clouds of 5, 300 and 20 000 points: segments byte for byte the single builds, even ascending bases from 0, a sentinel leaf
    behind each, the single builds' depths, the same bytes for 1 and 8 build threads; refusals by index."""
    exe, r = _harness(tmp_path, "plain", ["-O2", "-ffp-contract=off"])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forest harness ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_forest_packing_harness_under_asan_ubsan(tmp_path):
    exe, r = _harness(tmp_path, "asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forest harness ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
