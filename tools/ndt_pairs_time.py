#!/usr/bin/env python3
"""What scan-to-scan NDT odometry over a whole log costs (test_node.cpp:317-374: per scan SetInputTarget(last_cloud), ScanMatch(
current_cloud, SE3(), ...)), two ways, in one process:

  (A) what the library offered before the NDT pairs calls: per pair locgpu_ndt_set_target_cloud(scan i-1) +
      locgpu_ndt_align_cloud(scan i, identity) on one context, one pair after the other, on clouds that are resident already;
  (B) locgpu_ndt_set_target_set_batch(batch) + locgpu_ndt_align_pairs(batch, [-1, 0, 1, ...]) on the resident filtered batch, the
      ingest (device only: keys, one sort, voxels) and the alignment timed apart.

Inputs: `--scans` consecutive synthetic scans of 115 200 points, filtered at `--leaf` (0.5) by locgpu_batch_preprocess; NDT at
`--voxel` (the options' default 1.0), NEARBY6. (A) and (B) alternate, medians of `--reps` after `--warm` warm-up rounds, host wall time
round blocking calls (every one ends in a stream synchronisation). Before any timing the poses of (A) and (B) are compared. They are
not expected to be the same bits: a one-scan call and a 256-scan batch split a scan's sums into different groups (launch_ndt_accum's
points per thread follow the batch's size), and a different rounding of H and B can move an iteration count at the eps threshold. The
differences are reported; a pair beyond `POSE_TOL` whose iteration counts agree ends the run with an error. Each step runs under a
watchdog: a step that exceeds `--step-timeout` seconds ends the process with status 124 and nothing further is started.

    python3 tools/ndt_pairs_time.py --out build/ndt_pairs_time.json
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# FP64 sums of ~10^4 terms regrouped (relative 1e-16 · a few), through at most 20 Gauss–Newton solves of a well-conditioned 6 × 6
# system: orders of magnitude below this, which is itself 10^5 times below the project's pose bar of 1e-4.
POSE_TOL = 1e-9


def _expired(signum, frame):
    sys.stderr.write("ndt_pairs_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "ndt_pairs_time.json"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--first", type=int, default=3, help="id of the first scan of the circuit")
    ap.add_argument("--subsample", type=int, default=0, help="> 0: points kept of each raw scan (rehearsals)")
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--voxel", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    from loc_lib_amd import api, synth

    signal.signal(signal.SIGALRM, _expired)
    signal.alarm(a.step_timeout)
    raw = []
    for k in range(a.scans):
        s = synth.make_scan(a.first + k, subsample=a.subsample or None)
        x = np.zeros((len(s), 4), np.float32)
        x[:, :3] = s[:, :3]
        raw.append(x)
        if k % 32 == 31:
            print("generated %d scans" % (k + 1), flush=True)
    signal.alarm(0)
    res = dict(scans=a.scans, raw_points=int(sum(len(s) for s in raw)), leaf=a.leaf, voxel_size=a.voxel, library=os.environ.get("LOCGPU_LIB") or "in-tree")

    ctx_a, ctx_b = api.Context(0), api.Context(0)
    big = ctx_b.batch(raw)
    try:
        big.preprocess(a.leaf, out=ctx_b.batch_empty(a.scans, 1))
        raise SystemExit("a one-point dst cannot hold a filtered scan")
    except api.LocGpuError as e:
        need = e.counts
    small = ctx_b.batch_empty(a.scans, int(need.max()) + 64)
    big.preprocess(a.leaf, out=small)
    filtered = [np.ascontiguousarray(small.download_scan(k)) for k in range(a.scans)]
    big.close()
    res.update(filtered_points=int(need.sum()), filtered_max=int(need.max()), filtered_min=int(need.min()))
    print("filtered: %d points in %d scans (%d … %d)" % (res["filtered_points"], a.scans, res["filtered_min"], res["filtered_max"]), flush=True)
    clouds = []
    for f in filtered:  # (A) works on resident clouds: their upload is not part of what is timed
        x = np.zeros((len(f), 4), np.float32)
        x[:, :3] = np.asarray(f)[:, :3]
        clouds.append(api.Cloud(ctx_a, x))

    opts = api.ndt_opts(voxel_size=a.voxel, nearby_type=1)
    identity = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    target_of = np.arange(-1, a.scans - 1, dtype=np.int32)
    t = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        out = fn()
        t.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))
        return out

    def path_a():
        poses, iters, status = np.zeros((a.scans, 7)), np.zeros(a.scans, dtype=np.int64), np.zeros(a.scans, dtype=np.int64)
        poses[0] = identity
        for i in range(1, a.scans):
            ctx_a.ndt_set_target_cloud(clouds[i - 1], opts)
            poses[i], st = ctx_a.ndt_align_cloud(clouds[i], identity)
            iters[i], status[i] = st["iterations"], st["status"]
        return poses, iters, status

    def path_b():
        clock("B_set_ingest_from_batch", lambda: ctx_b.ndt_set_target_set_batch(small, opts))
        poses, stats = clock("B_align_pairs", lambda: ctx_b.ndt_align_pairs(small, target_of, None))
        return poses, np.array([s["iterations"] for s in stats]), np.array([s["status"] for s in stats])

    # faster and different is not faster: the poses first
    signal.alarm(a.step_timeout)
    pa, ia, sa = path_a()
    pb, ib, sb = path_b()
    signal.alarm(0)
    t.clear()
    diff = np.abs(pa - pb).max(axis=1)
    same_iters = ia == ib
    same_iters[0] = True  # row 0 has no target in (B) and is not aligned in (A)
    outside = (diff > POSE_TOL) & same_iters
    res.update(pose_max_abs_diff=float(diff.max()), pose_max_abs_diff_same_iterations=float(diff[same_iters].max()), pairs_equal=int((diff == 0).sum()),
               pairs_outside=int(outside.sum()), iterations_differ=int((~same_iters).sum()), status_differ=int((sa[1:] != sb[1:]).sum()),
               status_nonzero=int((sb[1:] != 0).sum()), iterations_mean=float(ib[1:].mean()), pose_tol=POSE_TOL, set_info_voxels=int(sum(ctx_b.ndt_set_info()["voxels"])))
    print("poses of (A) and (B): max |diff| %.3g (%.3g where the iteration counts agree), %d of %d rows equal, %d outside %.0e, iteration counts differ in %d, status in %d" %
          (res["pose_max_abs_diff"], res["pose_max_abs_diff_same_iterations"], res["pairs_equal"], a.scans, res["pairs_outside"], POSE_TOL, res["iterations_differ"],
           res["status_differ"]), flush=True)

    for r in range(a.warm + a.reps):
        signal.alarm(a.step_timeout)
        if r == a.warm:
            t.clear()
        clock("A_per_pair_set_target_and_align", path_a)
        clock("B_set_and_align_pairs", path_b)
        signal.alarm(0)
        print("round %d done" % r, flush=True)
    for name, v in t.items():
        res[name] = dict(wall_ms_median=round(float(np.median(v)), 3), wall_ms_min=round(min(v), 3), wall_ms_max=round(max(v), 3), reps=len(v))
        print("%-34s wall %9.3f ms (min %9.3f, max %9.3f)" % (name, res[name]["wall_ms_median"], res[name]["wall_ms_min"], res[name]["wall_ms_max"]), flush=True)
    res["A_over_B"] = round(res["A_per_pair_set_target_and_align"]["wall_ms_median"] / res["B_set_and_align_pairs"]["wall_ms_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if res["pairs_outside"]:
        raise SystemExit("poses of (A) and (B) differ by more than %.0e in %d pairs with equal iteration counts" % (POSE_TOL, res["pairs_outside"]))


if __name__ == "__main__":
    main()
