"""The rule that picks an alignment's compute stream (loc_lib_amd/csrc/stream_lease.hpp) on the CPU: tests/cpp/stream_lease_check.cpp,
exhaustive over loads 0-3 on three streams and every current stream — it keeps the current stream iff nobody else holds it, otherwise
returns a stream of minimal load, the lowest index on ties, never an index out of range — and the streaming rotation (four batches,
three alignments in flight) as bookkeeping. A stand-alone program under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_lease_rule_exhaustive(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "stream_lease_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "loc_lib_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "stream_lease_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "exhaustive: 192 cases OK" in r.stdout and "stream lease ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.count("rotation:") == 5
