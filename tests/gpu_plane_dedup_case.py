"""Helper of tests/test_gpu_plane_dedup.py: every result the test compares between LOCGPU_PLANE_DEDUP=1 and =0, computed in this
process from the inputs in the .npz named first and written to the .npz named second. The library reads the switch once per process,
so each setting is a process of its own."""
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


def main(inp, out):
    d = np.load(inp)
    ctx = api.Context(0)
    opts = api.icp_opts(method=api.P2PLANE)
    pose = d["pose"]
    res = {}
    ctx.icp_set_target(d["map"])
    # the designed scan at 1, 2 and 4 points per thread (the entries of a shared batch set the split, as test_points_per_thread_rungs has it)
    res["hb_single"] = np.concatenate([np.ravel(v) for v in ctx.icp_hb(d["scan"], pose, opts)]).astype(np.float64)
    for n_entries in d["rung_entries"]:
        b = ctx.batch_shared(d["scan"], int(n_entries))
        try:
            res["hb_x%d" % n_entries] = ctx.icp_hb_batch(b, np.stack([pose] * int(n_entries)), opts)
        finally:
            b.close()
    # ragged batch: the named counts beside an empty scan and the scan with non-finite points inside a run
    ragged = [d["ragged_%d" % i] for i in range(int(d["n_ragged"]))]
    b = ctx.batch(ragged)
    try:
        res["hb_ragged"] = ctx.icp_hb_batch(b, np.stack([pose] * len(ragged)), opts)
    finally:
        b.close()
    # alignments: one batch of four scans, and the same four as one pooled job
    scans = [d["align_%d" % i] for i in range(4)]
    inits = np.stack([d["init"]] * 4)
    b = ctx.batch(scans)
    try:
        poses, st = ctx.icp_align_batch(b, inits, opts)
    finally:
        b.close()
    res["batch_poses"], res["batch_stats"] = poses, _stats(st)
    pool = api.Pool(ctx, slots=4, max_points=max(len(s) for s in scans), scans_per_job=4, opts=opts)
    try:
        poses, st = pool.wait(pool.submit(scans, inits))
    finally:
        pool.close()
    res["pool_poses"], res["pool_stats"] = poses, _stats(st)
    # a target of four points: k = 5 fills no slot, every point has i < count and no list — at 1 and at 4 points per thread
    ctx.icp_set_target(d["map"][:4])
    head = np.ascontiguousarray(d["scan"][:int(d["nolist_points"])])
    res["hb_nolist_single"] = np.concatenate([np.ravel(v) for v in ctx.icp_hb(head, pose, opts)]).astype(np.float64)
    n_entries = int(d["nolist_entries"])
    b = ctx.batch_shared(head, n_entries)
    try:
        res["hb_nolist_x"] = ctx.icp_hb_batch(b, np.stack([pose] * n_entries), opts)
    finally:
        b.close()
    ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
