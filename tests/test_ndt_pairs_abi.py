"""Pairwise batch NDT on the host side: the voxel-set and pairs entry points are exported by liblocgpu.so, declared in
include/locgpu.h with the reference lines they stand for and bound in loc_lib_amd/api.py with the header's argument counts; a NULL
context is refused without a device; the status of a scan without a target is the ICP pairs' constant, not a second one; and the
host-side rules of a set (csrc/ndt_set_key.hpp: the key, the per-scan target words, the refusals decided before the device is
touched) pass their stand-alone harness, tests/cpp/ndt_set_key_check.cpp, with and without AddressSanitizer + UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loc_lib_amd", "csrc")
# name → the reference lines its own comment must cite
NAMES = {
    "locgpu_ndt_set_target_set": ("ndt_registration.cpp:65-85", "87-148", "test_node.cpp:317-374"),
    "locgpu_ndt_set_target_set_batch": ("ndt_registration.cpp:65-85", "87-148", "test_node.cpp:317-374"),
    "locgpu_ndt_set_info": ("ndt_registration.cpp:87-148",),
    "locgpu_ndt_set_dump": ("ndt_registration.cpp:87-148",),
    "locgpu_ndt_align_pairs": ("ndt_registration.cpp:238-261", ":374-464", "test_node.cpp:317-374", "test_node.cpp:348", "ndt_registration.cpp:435-436"),
    "locgpu_ndt_fitness_pairs": ("ndt_registration.cpp:374-464", "test_node.cpp:317-374"),
}
METHODS = ("ndt_set_target_set", "ndt_set_target_set_batch", "ndt_set_info", "ndt_set_dump", "ndt_align_pairs", "ndt_fitness_pairs")
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
    for method in METHODS:
        assert callable(getattr(api.Context, method)), method
    # the block stands behind the ICP pairs block and says what a set is, what it may hold, which calls a set context answers and
    # what is left out
    start = header.index("---- Pairwise batch NDT")
    assert start > header.index("LOCGPU_API int locgpu_icp_fitness_pairs(")
    block = header[start:header.index("LOCGPU_API int locgpu_ndt_set_target_set(")]
    for word in ("test_node.cpp:317-374", ":354", ":356", ":348", "ndt_registration.cpp:65-85, 87-148", "ndt_registration.cpp:238-261", ":374-464",
                 "target:16 | x:16 | y:16 | z:16", "65535", "2^15", "2^20", "exactly as it was", "incremental method is refused",
                 "locgpu_ndt_align*", "locgpu_ndt_hb*", "locgpu_ndt_scan_match", "locgpu_ndt_fitness*", "locgpu_ndt_init_search", "locgpu_ndt_dump",
                 "locgpu_pool_create", "matcher = 1", "re-check at submit", "ordinary again", "ICP target of the context is untouched", "locgpu_ndt_target_info",
                 "Not covered", "LOAM pairs", "incremental-NDT sets", "scan pools", "hipGraph", "sharded", "facade", "bench.py", "asynchronous"):
        assert word in block, word
    # the status of a scan without a target: the ICP pairs' constant, defined once, named in the stats struct's comment for both calls
    assert len(re.findall(r"#define\s+LOCGPU_STATUS_NO_PAIR_TARGET\b", header)) == 1
    m = re.search(r"#define\s+LOCGPU_STATUS_NO_PAIR_TARGET\s+(\d+)", header)
    assert m and int(m.group(1)) == api.STATUS_NO_PAIR_TARGET == 5
    assert "LOCGPU_STATUS_NO_PAIR_TARGET" in block
    stats = header[header.index("typedef struct locgpu_align_stats"):header.index("} locgpu_align_stats;")]
    assert "locgpu_ndt_align_pairs" in stats and "LOCGPU_STATUS_NO_PAIR_TARGET" in stats
    # the driver side is reused, not doubled: one status, one array of per-scan words
    context = open(os.path.join(CSRC, "context.hpp")).read()
    assert len(re.findall(r"\bd_pair_base;", context)) == 1 and len(re.findall(r"\bpair_skip;", context)) == 1
    # the new kernels are a file of their own, in the library's lists and outside the max-ilp objects
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bndt_pairs\.hip\b", mk, re.M) and re.search(r"^OBJS = .*\bndt_pairs\.o\b", mk, re.M)
    assert re.search(r"^HDRS = .*\bndt_pairs\.hpp\b.*\bndt_set_key\.hpp\b", mk, re.M)
    assert "ndt_pairs.o" not in re.search(r"^MAXILP_OBJS = (.*)$", mk, re.M).group(1)


def test_null_context_is_refused_without_a_device(api):
    L = api.lib()
    assert L.locgpu_ndt_set_target_set(None, None, None, 1, 16, None) == INVALID
    assert L.locgpu_ndt_set_target_set_batch(None, None, None) == INVALID
    assert L.locgpu_ndt_set_info(None, None, None, None) == INVALID
    assert L.locgpu_ndt_set_dump(None, 0, None, None, None, 0, None) == INVALID
    assert L.locgpu_ndt_align_pairs(None, None, None, None, None, None) == INVALID
    assert L.locgpu_ndt_fitness_pairs(None, None, None, None, None) == INVALID


def _harness(tmp_path, tag, flags):
    exe = str(tmp_path / ("ndt_set_key_" + tag))
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ndt_set_key_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return exe, r


def test_set_key_harness(tmp_path):
    """Key round trips at the corners of the range and of the target index, never the empty marker, linear across the range boundary
    (a centre one voxel outside keeps exactly its one neighbour inside); target words from target_of for NDT (the index) and ICP (a
    base table), refusals by entry with the outputs untouched; the ingest's refusals by index."""
    exe, r = _harness(tmp_path, "plain", ["-O2"])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ndt set key harness ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_set_key_harness_under_asan_ubsan(tmp_path):
    exe, r = _harness(tmp_path, "asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ndt set key harness ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
