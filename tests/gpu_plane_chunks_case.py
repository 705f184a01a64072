"""Helper of tests/test_gpu_plane_chunks.py: every result the test compares between the default plane kernel (lists parked in the
plane table, runs from the search stage's flags), LOCGPU_PLANE_RUNFLAGS=0 (runs found from the lists) and LOCGPU_PLANE_DEDUP=0 (a fit
per point), computed in this process from the inputs in the .npz named first and written to the .npz named second. The library reads
the switches once per process, so each setting is a process of its own. Third argument: "all", or "designed" (the designed scan at
four points per thread alone)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from loc_lib_amd import api  # noqa: E402

REPEATS = 10


def _shared(ctx, scan, n_entries, pose, opts, res, key, repeats=1, nn=False):
    b = ctx.batch_shared(np.ascontiguousarray(scan), int(n_entries))
    try:
        poses = np.stack([pose] * int(n_entries))
        runs = [ctx.icp_hb_batch(b, poses, opts) for _ in range(repeats)]
        res["hb_" + key] = runs[0]
        if repeats > 1:
            res["hb_repeats_" + key] = np.stack(runs)
        words, written = ctx.debug_batch_run_flags(b)
        res["written_" + key], res["flags_" + key] = np.array(written), words
        if nn:
            res["nn_" + key] = ctx.debug_batch_nn(b, 5)
    finally:
        b.close()


def _ragged(ctx, d, rung, pose, opts, res):
    scans = [d["ragged%d_%d" % (rung, i)] for i in range(int(d["n_ragged%d" % rung]))]
    b = ctx.batch(scans)
    try:
        res["hb_ragged%d" % rung] = ctx.icp_hb_batch(b, np.stack([pose] * len(scans)), opts)
        words, written = ctx.debug_batch_run_flags(b)
        res["written_ragged%d" % rung], res["flags_ragged%d" % rung] = np.array(written), words
    finally:
        b.close()


def main(d, res, what):
    ctx = api.Context(0)
    opts = api.icp_opts(method=api.P2PLANE)
    pose = d["pose"]
    ctx.icp_set_target(d["map"])
    ctx.search_stats_read(reset=True)  # the first call switches the counters on
    entries = {int(r): int(n) for r, n in d["rung_entries"]}
    _shared(ctx, d["scan"], entries[4], pose, opts, res, "x4", repeats=REPEATS if what == "all" else 1)
    if what == "all":
        _shared(ctx, d["scan"], entries[2], pose, opts, res, "x2")
        _shared(ctx, d["scan"], entries[1], pose, opts, res, "x1")
        st = ctx.search_stats_read(reset=True)
        res["stats"] = np.array([st["searched"], st["redone"], st["walked"]], dtype=np.int64)
        _ragged(ctx, d, 1, pose, opts, res)
        _ragged(ctx, d, 4, pose, opts, res)
        st = ctx.search_stats_read(reset=True)
        res["stats_ragged"] = np.array([st["searched"], st["redone"], st["walked"]], dtype=np.int64)
        # the same runs over 300 clusters: the deep pass of the search stage makes leaders of its own
        ctx.icp_set_target(d["wide_map"])
        ctx.search_stats_read(reset=True)
        _shared(ctx, d["wide_scan"], entries[4], pose, opts, res, "wide")
        st = ctx.search_stats_read(reset=True)
        res["stats_wide"] = np.array([st["searched"], st["redone"], st["walked"]], dtype=np.int64)
        # four map points: no query has a list
        ctx.icp_set_target(d["map"][:4])
        points, e1, e4 = (int(v) for v in d["nolist"])
        _shared(ctx, d["scan"][:points], e1, pose, opts, res, "nolist1", nn=True)
        _shared(ctx, d["scan"][:points], e4, pose, opts, res, "nolist4")
    ctx.close()


if __name__ == "__main__":
    data, out = np.load(sys.argv[1]), {}
    main(data, out, sys.argv[3])
    np.savez(sys.argv[2], **out)
