"""Helper of tests/test_gpu_walk_prefix.py: one search stage per case of the .npz named first, in this process (the library reads
LOCGPU_FAST_STACK once per process), results to the .npz named second. Third argument: comma-separated case names.

Per case `c` the input holds map_c, the pose, and either scan_c + entries_c (a shared batch: every entry reads the one scan) or
ragged_c_0 … ragged_c_{n-1} (a batch of scans of different lengths). Output per case and k in (5, 1): nn{k}_c = the neighbour lists of
the first and the last entry (shared) or of every scan (ragged), same{k}_c = whether every entry of a shared batch got the first
one's lists, written_c = whether the k = 5 stage wrote run flags (the 64-lane walk kernel alone does), flags_c = the flag words."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from loc_lib_amd import api  # noqa: E402


def run_case(ctx, d, c, res):
    ctx.icp_set_target(d["map_" + c])
    pose = d["pose"]
    if "scan_" + c in d:
        n = int(d["entries_" + c])
        b = ctx.batch_shared(np.ascontiguousarray(d["scan_" + c]), n)
    else:
        scans = [d["ragged_%s_%d" % (c, i)] for i in range(int(d["n_ragged_" + c]))]
        n = len(scans)
        b = ctx.batch(scans)
    try:
        for method, k in ((api.P2PLANE, 5), (api.P2P, 1)):
            ctx.icp_hb_batch(b, np.stack([pose] * n), api.icp_opts(method=method))
            nn = ctx.debug_batch_nn(b, k)
            if "scan_" + c in d:
                res["same%d_%s" % (k, c)] = np.array(bool((nn == nn[0]).all()))
                res["nn%d_%s" % (k, c)] = nn[[0, n - 1]]
            else:
                res["nn%d_%s" % (k, c)] = nn
            if k == 5:
                words, written = ctx.debug_batch_run_flags(b)
                res["written_" + c] = np.array(written)
                res["flags_" + c] = words
    finally:
        b.close()


if __name__ == "__main__":
    data, out = np.load(sys.argv[1]), {}
    ctx = api.Context(0)
    for case in sys.argv[3].split(","):
        run_case(ctx, data, case, out)
    ctx.close()
    np.savez(sys.argv[2], **out)
