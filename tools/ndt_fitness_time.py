"""Times locgpu_ndt_fitness_batch on the bench batch (256 scans of 115 200 points against the NDT table of the 10 M-point map) beside
ONE launch of ndt_accum_kernel on the same batch in the same process (profiles/ndt_fitness.md).

The accumulate launch is timed by the library's own stage events (locgpu_profile_enable) around an alignment limited to one iteration,
and by the host clock around that call; the score has no stage events, so it is timed by the host clock around the blocking call
(state upload, the score kernel, the sum kernel, read-back and synchronisation included): the two host-clock figures compare like with
like, the event figure is the kernel alone.

    python tools/ndt_fitness_time.py [--scans 256] [--map-points 10000000] [--repeat 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--map-points", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from loc_lib_amd import api, synth

    m = synth.make_map(args.map_points)
    ids = [i % 256 for i in range(args.scans)]
    scan_of = {i: synth.make_scan(i) for i in sorted(set(ids))}
    scans = [scan_of[i] for i in ids]
    inits = np.stack([synth.make_pose(i)[1] for i in ids])
    ctx = api.Context(0)
    res = dict(scans=args.scans, points_per_scan=len(scans[0]), map_points=args.map_points)
    try:
        b = ctx.batch(scans)
        # one Gauss–Newton iteration = one ndt_accum_kernel launch over every scan of the batch
        ctx.ndt_set_target(m, api.ndt_opts(max_iteration=1))
        res["voxels"] = ctx.ndt_target_info()["num_voxels"]
        ctx.ndt_align_batch(b, inits)  # warm-up
        wall = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            ctx.ndt_align_batch(b, inits)
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        for _ in range(args.repeat):
            ctx.ndt_align_batch(b, inits)
        prof = ctx.profile_read(reset=True)
        ctx.profile_enable(False)
        res["accum_kernel_ms_events"] = prof["accum_ms"]
        res["accum_launches_timed"] = prof["accum_n"]
        res["one_iteration_call_ms_host"] = dict(min=min(wall), median=float(np.median(wall)))
        ctx.ndt_fitness_batch(b, inits)  # warm-up
        wall = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fit = ctx.ndt_fitness_batch(b, inits)
            wall.append((time.perf_counter() - t0) * 1e3)
        res["fitness_call_ms_host"] = dict(min=min(wall), median=float(np.median(wall)))
        res["ratio_host_min"] = min(wall) / res["one_iteration_call_ms_host"]["min"]
        res["mean_inlier_ratio"] = float(np.mean([f["inliers"] / f["finite_points"] for f in fit]))
        b.close()
    finally:
        ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
