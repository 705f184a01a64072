"""The device tree build on the host side: its entry points are exported by liblocgpu.so, declared in include/locgpu.h
with the reference lines they relate to and bound in loc_lib_amd/api.py with the header's argument counts; a NULL context is refused
without a device; the layout rules and the sequential node split shared with the kernel (csrc/forest_plan.hpp) pass their stand-alone
harness, tests/cpp/forest_device_plan_check.cpp, with and without AddressSanitizer + UBSan (that harness does not run the kernel's
cooperative path — tests/test_gpu_forest_device.py does); and the fixtures of the GPU tests are what those tests need them to be."""
import os
import re
import subprocess

import numpy as np
import pytest

import forest_device_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loc_lib_amd", "csrc")
NAMES = {
    "locgpu_icp_set_target_forest_device": ("icp_registration.cpp:9-29", "test_node.cpp:256-315"),
    "locgpu_icp_set_target_cloud_device": ("icp_registration.cpp:9-29", "lio.cpp:296-305"),
    "locgpu_icp_device_build_info": ("kdtree.cpp:58-94",),
    "locgpu_debug_tree_read": ("kdtree.cpp:10-31",),
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
    for method in ("icp_set_target_forest_device", "icp_set_target_cloud_device", "icp_device_build_info", "debug_tree_read"):
        assert callable(getattr(api.Context, method)), method
    start = header.index("---- The ICP target's KD-trees built on the device")
    block = header[start:header.index("LOCGPU_API int locgpu_icp_set_target_forest_device(")]
    for word in ("DESIGN.md §25", "byte for byte", "degenerate", "host path", "exactly as", "LOCGPU_ERR_DEPTH", "Opt-in", "Not covered", "facade", "bench.py", "sharded"):
        assert word in block, word
    # the sources are listed where the build and resource_usage.sh look for them
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bforest_build\.hip\b", mk, re.M) and re.search(r"^OBJS = .*\bforest_build\.o\b", mk, re.M)
    assert re.search(r"^HDRS = .*\bforest_plan\.hpp\b.*\bforest_build\.hpp\b", mk, re.M)


def test_null_context_is_refused_without_a_device(api):
    L = api.lib()
    out = np.full(8, 7, dtype=np.int64)
    assert L.locgpu_icp_set_target_forest_device(None, None) == INVALID
    assert L.locgpu_icp_set_target_cloud_device(None, None) == INVALID
    assert L.locgpu_icp_device_build_info(None, out.ctypes.data) == INVALID
    assert L.locgpu_debug_tree_read(None, None, 0, None, 0) == INVALID
    assert (out == 7).all()


def _harness(tmp_path, tag, flags):
    exe = str(tmp_path / ("forest_device_plan_" + tag))
    cmd = ["g++", "-std=c++17"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "forest_device_plan_check.cpp"), os.path.join(CSRC, "kdtree_build.cpp"), "-o", exe,
                                           "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return exe, r


def test_plan_harness(tmp_path):
    """A level-synchronous host driver over forest_plan.hpp — bases and pads, child slots, leaf positions, slot encoding, the sequential
    split — against build_packed_forest byte for byte: twenty trees of 1 … 20 000 points, the special clouds included; leaf slots, depths
    and `bounded` against the single builds; a duplicated point is flagged degenerate."""
    exe, r = _harness(tmp_path, "plain", ["-O2", "-ffp-contract=off"])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forest device plan ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_plan_harness_under_asan_ubsan(tmp_path):
    exe, r = _harness(tmp_path, "asan", ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forest device plan ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def test_gpu_fixtures_have_no_degenerate_split(api, synth):
    """Every target the GPU tests build on the device — the duplicate case excepted — makes a host tree of exactly 3n − 1 slots: no
    degenerate split, so the device path cannot hide behind its fallback. The duplicate case does have one; the chain is deeper than 64 levels."""
    world = cases.pair_world(synth)
    clouds = [c for _, c in cases.forest_targets(synth)] + world["targets"] + cases.single_clouds(synth) + cases.with_huge() + [cases.deep_chain()]
    for c in clouds:
        slots, info = cases.host_tree(api, c)
        assert len(slots) == 3 * len(c) - 1 and info[0] == len(c), (len(c), len(slots))
    dup = cases.with_duplicate()
    assert [len(cases.host_tree(api, c)[0]) == 3 * len(c) - 1 for c in dup] == [True, False, True]
    chain = cases.deep_chain()
    assert 64 < cases.host_tree(api, chain)[1][2] <= len(chain) == 72
    sizes = sorted(len(c) for _, c in cases.forest_targets(synth))
    for want in (1, 2, 3, 5, 63, 64, 65, cases.LANE_LEN - 1, cases.LANE_LEN, cases.LANE_LEN + 1, cases.TILE - 1, cases.TILE, cases.TILE + 1, 2049, 4000, 20000):
        assert want in sizes, want


def test_offset_cloud_catches_reassociation(api):
    """For the cloud 5000 m from the origin, numpy's pairwise float32 sum of the root's points on the split axis differs from the
    float32 sum in index order — a build that reassociates the root's sum would move its threshold."""
    c = cases.offset()
    slots, _ = cases.host_tree(api, c)
    axis = int(slots[0] >> np.uint64(62))
    assert axis in (0, 1)
    col = np.ascontiguousarray(c[:, axis])
    in_order = np.float32(0.0)
    for v in col:
        in_order = np.float32(in_order + v)
    pairwise = np.sum(col, dtype=np.float32)
    assert in_order != pairwise, (in_order, pairwise)
    th = np.array([slots[0] & np.uint64(0xFFFFFFFF)], dtype=np.uint64).astype(np.uint32).view(np.float32)[0]
    assert th == np.float32(in_order / np.float32(len(col)))  # the root's threshold IS the index-order mean
    assert th != np.float32(pairwise / np.float32(len(col)))
