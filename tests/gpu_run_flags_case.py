"""Helper of tests/test_gpu_run_flags.py: every result the test compares between LOCGPU_PLANE_RUNFLAGS=1 and =0, computed in this
process from the inputs in the .npz named first and written to the .npz named second. The library reads the switch (and
LOCGPU_FAST_STACK) once per process, so each setting is a process of its own. Third argument: "main" or "far"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from loc_lib_amd import api  # noqa: E402


def _stats(st):
    return np.array([[s["iterations"], s["converged"], s["status"], s["last_effective_num"]] for s in st], dtype=np.int64)


def _hb_shared(ctx, scan, n_entries, pose, opts, res, key, lists=False):
    """H/B of n_entries shared entries of `scan` at `pose`; with it whether the stage wrote run flags and, lists=True, the flag words,
    the neighbour lists and the stage's counters."""
    b = ctx.batch_shared(np.ascontiguousarray(scan), int(n_entries))
    try:
        ctx.search_stats_read(reset=True)
        res["hb_" + key] = ctx.icp_hb_batch(b, np.stack([pose] * int(n_entries)), opts)
        words, written = ctx.debug_batch_run_flags(b)
        st = ctx.search_stats_read(reset=True)
        res["written_" + key] = np.array(written)
        res["stats_" + key] = np.array([st["searched"], st["redone"], st["walked"]], dtype=np.int64)
        if lists:
            res["flags_" + key] = words
            res["nn_" + key] = ctx.debug_batch_nn(b, 5)
    finally:
        b.close()


def main_case(d, res):
    ctx = api.Context(0)
    opts = api.icp_opts(method=api.P2PLANE)
    pose = d["pose"]
    ctx.icp_set_target(d["map"])
    ctx.search_stats_read(reset=True)  # the first call switches the counters on
    # the designed scan alone: the 16-lane walk kernel, which writes no flags
    b = ctx.batch([d["scan"]])
    try:
        res["hb_single"] = ctx.icp_hb_batch(b, pose[None], opts)
        res["written_single"] = np.array(ctx.debug_batch_run_flags(b)[1])
    finally:
        b.close()
    # … and as shared batches: 2 and 4 points per thread (90, 179 entries), 1 point per thread (33 entries of its first 4 000 points)
    _hb_shared(ctx, d["scan"], 90, pose, opts, res, "x90", lists=True)
    _hb_shared(ctx, d["scan"], 179, pose, opts, res, "x179")
    _hb_shared(ctx, d["scan"][:4000], 33, pose, opts, res, "x33")
    # the grid search writes no flags
    _hb_shared(ctx, d["scan"], 90, pose, api.icp_opts(method=api.P2PLANE, search_mode=api.SEARCH_GRID_EXACT), res, "grid")
    # ragged batch, padded past 2 048 walk waves
    ragged = [d["ragged_%d" % i] for i in range(int(d["n_ragged"]))]
    b = ctx.batch(ragged)
    try:
        res["hb_ragged"] = ctx.icp_hb_batch(b, np.stack([pose] * len(ragged)), opts)
        res["written_ragged"] = np.array(ctx.debug_batch_run_flags(b)[1])
    finally:
        b.close()
    # alignments: one batch, the same scans as one pooled job, and the batch under graph capture. eps is far below the reference's
    # 1e-2, so that scans stay open behind the first chunk of iterations, where the launches go over `active` lists — the pool looks at
    # the flags every second iteration
    n_align = int(d["n_align"])
    scans = [d["align_%d" % i] for i in range(n_align)]
    inits = d["inits"]
    opts = api.icp_opts(method=api.P2PLANE, eps=1e-11)
    b = ctx.batch(scans)
    try:
        poses, st = ctx.icp_align_batch(b, inits, opts)
        res["batch_poses"], res["batch_stats"] = poses, _stats(st)
        ctx.graph_enable(True)
        try:
            poses, st = ctx.icp_align_batch(b, inits, opts)
        finally:
            ctx.graph_enable(False)
        res["graph_poses"], res["graph_stats"] = poses, _stats(st)
    finally:
        b.close()
    opts = api.icp_opts(method=api.P2PLANE)
    pool = api.Pool(ctx, slots=n_align, max_points=max(len(s) for s in scans), scans_per_job=n_align, chunk=2, opts=api.icp_opts(method=api.P2PLANE, eps=1e-11))
    try:
        poses, st = pool.wait(pool.submit(scans, inits))
    finally:
        pool.close()
    res["pool_poses"], res["pool_stats"] = poses, _stats(st)
    # a lattice map: ties send many queries to the in-wave exact walk and the redo kernel
    ctx.icp_set_target(d["lattice"])
    _hb_shared(ctx, d["lattice_scan"], 40, d["lattice_pose"], opts, res, "lattice", lists=True)
    # a map of 120 points (no query outgrows the stack rows) under pairs of points 5 cm apart: one set, often in two distance orders
    ctx.icp_set_target(d["small_map"])
    _hb_shared(ctx, d["order_scan"], 33, pose, opts, res, "order", lists=True)
    # a target of four points: no query has a list — every point is flagged a leader and none fits; 1 and 4 points per thread
    ctx.icp_set_target(d["map"][:4])
    head = d["scan"][:int(d["nolist_points"])]
    _hb_shared(ctx, head, 90, pose, opts, res, "nolist_x90", lists=True)
    _hb_shared(ctx, head, int(d["nolist_entries"]), pose, opts, res, "nolist_x")
    ctx.close()


def far_case(d, res):
    """Run under LOCGPU_FAST_STACK=12: a far pose against a larger map with a lattice in it — deep pass and ties are common."""
    ctx = api.Context(0)
    ctx.icp_set_target(d["far_map"])
    ctx.search_stats_read(reset=True)
    _hb_shared(ctx, d["far_scan"], 40, d["far_pose"], api.icp_opts(method=api.P2PLANE), res, "far", lists=True)
    ctx.close()


if __name__ == "__main__":
    data, out = np.load(sys.argv[1]), {}
    (far_case if sys.argv[3] == "far" else main_case)(data, out)
    np.savez(sys.argv[2], **out)
