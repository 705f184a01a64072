#!/usr/bin/env python3
"""What scan-to-scan odometry over a whole log costs (test_node.cpp:256-315: per scan SetInputTarget(last_cloud), ScanMatch(current_cloud,
SE3(), ...)), two ways, in one process:

  (A) what the library offered before the pairs calls: per pair locgpu_icp_set_target(scan i-1) + locgpu_icp_align(scan i, identity) on
      one context, one pair after the other, from host arrays;
  (B) locgpu_icp_set_target_forest_batch(batch) + locgpu_icp_align_pairs(batch, [-1, 0, 1, ...]) on the resident filtered batch.
      Reported apart: the forest ingest (device-to-host copy of the scans, host build of all trees, one host-to-device copy) and the
      alignment; and the ingest from host arrays (locgpu_icp_set_target_forest), which has no device-to-host copy. LOCGPU_FOREST_TIMES=1
      makes the library print the ingest's own phases (host build | device buffers + H2D) on stderr.

Inputs: `--scans` consecutive synthetic scans of 115 200 points, filtered at `--leaf` (0.5) by locgpu_batch_preprocess; point-to-plane,
the options' defaults. (A) and (B) alternate, medians of `--reps` after `--warm` warm-up rounds, host wall time round blocking calls
(every one ends in a stream synchronisation). Before any timing the poses of (A) and (B) are compared: equal, or within the 7e-15 that
a batch's split of its sums explains (a one-scan call and a 256-scan batch add a scan's partial sums in different groups). Each step
runs under a watchdog: a step that exceeds `--step-timeout` seconds ends the process with status 124 and nothing further is started.

    python3 tools/pairs_time.py --out build/pairs_time.json
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
POSE_TOL = 7e-15


def _expired(signum, frame):
    sys.stderr.write("pairs_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pairs_time.json"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--first", type=int, default=3, help="id of the first scan of the circuit")
    ap.add_argument("--subsample", type=int, default=0, help="> 0: points kept of each raw scan (rehearsals)")
    ap.add_argument("--leaf", type=float, default=0.5)
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
    res = dict(scans=a.scans, raw_points=int(sum(len(s) for s in raw)), leaf=a.leaf, library=os.environ.get("LOCGPU_LIB") or "in-tree")

    ctx_a, ctx_b = api.Context(0), api.Context(0)
    big = ctx_b.batch(raw)
    try:
        big.preprocess(a.leaf, out=ctx_b.batch_empty(a.scans, 1))
        raise SystemExit("a one-point dst cannot hold a filtered scan")
    except api.LocGpuError as e:
        need = e.counts
    small = ctx_b.batch_empty(a.scans, int(need.max()) + 64)
    big.preprocess(a.leaf, out=small)
    filtered = [np.ascontiguousarray(small.download_scan(k)[:, :3]) for k in range(a.scans)]
    big.close()
    res.update(filtered_points=int(need.sum()), filtered_max=int(need.max()), filtered_min=int(need.min()))
    print("filtered: %d points in %d scans (%d … %d)" % (res["filtered_points"], a.scans, res["filtered_min"], res["filtered_max"]), flush=True)

    opts = api.icp_opts(method=api.P2PLANE)
    identity = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    target_of = np.arange(-1, a.scans - 1, dtype=np.int32)
    t = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        out = fn()
        t.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))
        return out

    def path_a():
        poses, iters = np.zeros((a.scans, 7)), np.zeros(a.scans, dtype=np.int64)
        poses[0] = identity
        for i in range(1, a.scans):
            ctx_a.icp_set_target(filtered[i - 1])
            poses[i], st = ctx_a.icp_align(filtered[i], identity, opts)
            iters[i] = st["iterations"]
        return poses, iters

    def path_b():
        clock("B_forest_ingest_from_batch", lambda: ctx_b.icp_set_target_forest_batch(small))
        poses, stats = clock("B_align_pairs", lambda: ctx_b.icp_align_pairs(small, target_of, None, opts))
        return poses, np.array([s["iterations"] for s in stats])

    # faster and different is not faster: the poses first
    signal.alarm(a.step_timeout)
    pa, ia = path_a()
    pb, ib = path_b()
    signal.alarm(0)
    t.clear()
    diff = np.abs(pa - pb).max(axis=1)
    res.update(pose_max_abs_diff=float(diff.max()), pairs_equal=int((diff == 0).sum()), pairs_outside=int((diff > POSE_TOL).sum()),
               iterations_differ=int((ia != ib).sum()), iterations_mean=float(ib[1:].mean()), pose_tol=POSE_TOL)
    print("poses of (A) and (B): max |diff| %.3g, %d of %d rows equal, %d outside %.0e, iteration counts differ in %d" %
          (res["pose_max_abs_diff"], res["pairs_equal"], a.scans, res["pairs_outside"], POSE_TOL, res["iterations_differ"]), flush=True)

    for r in range(a.warm + a.reps):
        signal.alarm(a.step_timeout)
        if r == a.warm:
            t.clear()
        clock("A_per_pair_set_target_and_align", path_a)
        clock("B_forest_and_align_pairs", path_b)
        clock("B_forest_ingest_from_host", lambda: ctx_b.icp_set_target_forest(filtered))
        signal.alarm(0)
        print("round %d done" % r, flush=True)
    for name, v in t.items():
        res[name] = dict(wall_ms_median=round(float(np.median(v)), 3), wall_ms_min=round(min(v), 3), wall_ms_max=round(max(v), 3), reps=len(v))
        print("%-34s wall %9.3f ms (min %9.3f, max %9.3f)" % (name, res[name]["wall_ms_median"], res[name]["wall_ms_min"], res[name]["wall_ms_max"]), flush=True)
    res["A_over_B"] = round(res["A_per_pair_set_target_and_align"]["wall_ms_median"] / res["B_forest_and_align_pairs"]["wall_ms_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if res["pairs_outside"]:
        raise SystemExit("poses of (A) and (B) differ by more than %.0e in %d pairs" % (POSE_TOL, res["pairs_outside"]))


if __name__ == "__main__":
    main()
