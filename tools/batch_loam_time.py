#!/usr/bin/env python3
"""What Lio::AddCloud(FullCloudPtr)'s step (lio.cpp:311-410: feature picker, voxel filter of both feature clouds, LOAM match) costs on a
whole batch of raw scans, two ways, in one process:

  (A) per scan, what the library offered before locgpu_batch_loam_extract: Cloud.upload → locgpu_cloud_loam_extract → two
      locgpu_cloud_voxel_filter (in place) → locgpu_loam_scan_match_cloud;
  (B) one locgpu_batch_upload_async + wait of the raw scans → locgpu_batch_loam_extract → two in-place locgpu_batch_preprocess →
      locgpu_loam_align_batches;
  and, of (B), the picker pass alone on scans that are already resident (`--only picker` is the run to put under a kernel trace),
  the two in-place filters alone and the match alone.

Inputs: 256 scans of 115 200 points (64 rings × 1800, ring = index // 1800; `--distinct` different synthetic scans, repeated in turn)
at leaf 0.5; the maps are the picker's unfiltered features of synth.make_scan(0) at its true pose. Every figure is the median of
`--reps` repetitions after `--warm` warm-up runs, as host wall time and as the time between two HIP events recorded on the null stream
round the (blocking) calls. After (A) and (B) their poses are compared (a batch splits its partial sums by the batch's shape, so last
bits may differ between a batch and a single-scan call: the largest difference is reported, not asserted to be zero), and the feature
batches of (B) are compared byte for byte with (A)'s filtered clouds. Each step runs under a watchdog of its own: a step that exceeds
`--step-timeout` seconds ends the process with status 124 and nothing further is started.

    python3 tools/batch_loam_time.py --out build/batch_loam_time.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from batch_preprocess_time import HipEvents  # noqa: E402

NUM_SCAN, RING_LEN = 64, 1800


def _expired(signum, frame):
    sys.stderr.write("batch_loam_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def timed(name, fn, ev, warm, reps, limit, res):
    signal.signal(signal.SIGALRM, _expired)
    signal.alarm(limit)
    for _ in range(warm):
        fn()
    wall, dev = [], []
    for _ in range(reps):
        ev.start()
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(ev.stop_ms())
    signal.alarm(0)
    res[name] = dict(wall_ms_median=round(float(np.median(wall)), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                     hip_event_ms_median=round(float(np.median(dev)), 3), reps=reps)
    print("%-34s wall %9.3f ms (min %9.3f, max %9.3f)   HIP events %9.3f ms" % (name, res[name]["wall_ms_median"], res[name]["wall_ms_min"],
                                                                                 res[name]["wall_ms_max"], res[name]["hip_event_ms_median"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "batch_loam_time.json"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--only", default="", help="comma-separated subset of A,B,picker,filters,match (default: all)")
    a = ap.parse_args()
    only = set(x for x in a.only.split(",") if x)
    from loc_lib_amd import api, synth

    def raw(i):
        s = synth.make_scan(i)
        x = np.zeros((len(s), 4), np.float32)
        x[:, :3] = s[:, :3]
        return x

    distinct = [raw(1 + k) for k in range(a.distinct)]
    inits = [synth.make_pose(1 + k)[1] for k in range(a.distinct)]
    n_pts = len(distinct[0])
    assert n_pts == NUM_SCAN * RING_LEN and all(len(x) == n_pts for x in distinct)
    ring = (np.arange(n_pts) // RING_LEN).astype(np.uint8)
    scans = [distinct[i % a.distinct] for i in range(a.scans)]
    rings = [ring] * a.scans
    poses = np.array([inits[i % a.distinct] for i in range(a.scans)], dtype=np.float64)
    res = dict(scans=a.scans, distinct=a.distinct, points=a.scans * n_pts, leaf=a.leaf, num_scan=NUM_SCAN)

    ctx = api.Context(0)
    ev = HipEvents()
    h = api.Loam()
    c0 = api.Cloud(ctx, raw(0))
    e0, s0 = c0.loam_extract(ring, NUM_SCAN)
    truth0 = synth.make_pose(0)[0]
    e0.transform(truth0, out=e0)
    s0.transform(truth0, out=s0)
    h.set_target_cloud(e0, s0)
    res.update(edge_map_points=len(e0), surf_map_points=len(s0))

    marsh = api.MarshalledScans(scans)
    big = ctx.batch_empty(a.scans, n_pts)
    edge_b, surf_b = ctx.batch_empty(a.scans, NUM_SCAN * 6 * 20), ctx.batch_empty(a.scans, n_pts)
    big.upload_async(marsh)
    big.upload_wait()
    c_raw = api.Cloud(ctx)
    out_a = dict(poses=np.zeros((a.scans, 7)), edge=[None] * a.scans, surf=[None] * a.scans)
    out_b = dict(poses=None)

    def step_a(keep=False):
        for i, s in enumerate(scans):
            c_raw.upload(s)
            edge, surf = c_raw.loam_extract(ring, NUM_SCAN)
            edge.voxel_filter(a.leaf, out=edge)
            surf.voxel_filter(a.leaf, out=surf)
            out_a["poses"][i], _ = h.scan_match_cloud(edge, surf, poses[i])
            if keep:
                out_a["edge"][i], out_a["surf"][i] = edge.download(), surf.download()
            edge.close()
            surf.close()

    def picker():
        return big.loam_extract(rings, NUM_SCAN, edge_b, surf_b)

    def filters():
        edge_b.preprocess(a.leaf)
        surf_b.preprocess(a.leaf)

    def match():
        out_b["poses"], out_b["stats"] = h.align_batches(edge_b, surf_b, poses)

    def step_b():
        big.upload_async(marsh)
        big.upload_wait()
        picker()
        filters()
        match()

    if not only or "A" in only:
        timed("A_per_scan_pick_filter_match", step_a, ev, min(a.warm, 1), a.reps, a.step_timeout, res)
    if not only or "B" in only:
        timed("B_batch_upload_pick_filter_match", step_b, ev, a.warm, a.reps, a.step_timeout, res)
    if not only or {"A", "B"} <= only:
        signal.alarm(a.step_timeout)
        step_a(keep=True)
        step_b()
        signal.alarm(0)
        res["features_equal"] = all(out_a["edge"][k][:, :3].tobytes() == edge_b.download_scan(k)[:, :3].tobytes() and
                                    out_a["surf"][k][:, :3].tobytes() == surf_b.download_scan(k)[:, :3].tobytes() for k in range(a.scans))
        res["poses_max_abs_diff"] = float(np.abs(out_a["poses"] - out_b["poses"]).max())
        res["status_nonzero_B"] = int(sum(1 for st in out_b["stats"] if st["status"] != 0))
        print("filtered features of (A) and (B) equal, all %d scans: %s; largest pose difference %.3e" %
              (a.scans, res["features_equal"], res["poses_max_abs_diff"]), flush=True)
        assert res["features_equal"]
    if not only or "picker" in only:
        timed("picker_only_resident", picker, ev, a.warm, a.reps, a.step_timeout, res)
        ne, ns, _ = picker()
        ms = res["picker_only_resident"]["hip_event_ms_median"]
        res["picker_only_resident"].update(slots_per_s=round(a.scans * n_pts / (ms * 1e-3), 1), edge_points=int(ne.sum()), surf_points=int(ns.sum()))
    if not only or "filters" in only:
        def pick_and_filter():
            picker()
            filters()
        timed("picker_plus_two_filters_resident", pick_and_filter, ev, a.warm, a.reps, a.step_timeout, res)
    if not only or "match" in only:
        picker()
        filters()
        timed("align_batches_of_filtered", match, ev, a.warm, a.reps, a.step_timeout, res)
        res["align_batches_of_filtered"]["iterations"] = [int(st["iterations"]) for st in out_b["stats"][:a.distinct]]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
