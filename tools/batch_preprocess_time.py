#!/usr/bin/env python3
"""What the reference's front-end (RemoveNanPoint → VoxelFilter::Filter, loc.cpp:217-218) costs on a whole batch, two ways, in one process:

  (A) what the library offered before locgpu_batch_preprocess, host to host: per scan Cloud.upload → remove_nan → voxel_filter →
      download, then locgpu_batch_upload_async + locgpu_batch_upload_wait of the filtered scans into a small batch;
  (B) locgpu_batch_upload_async + wait of the raw scans into a full-size batch, then locgpu_batch_preprocess into a small batch
      (also reported: the preprocess call alone, on scans that are already resident);
  and, beside both, one locgpu_icp_align_batch (point-to-plane) of the filtered batch, so that the front-end's share of a step shows.

Inputs: 256 scans of 115 200 points (`--distinct` different synthetic scans, repeated in turn; 1 % of the points made NaN) at
leaf = 1.0 (cur_scan_filter, loc.cpp:218) against a 2 M-point map. Every figure is the median of `--reps` repetitions after `--warm`
warm-up runs, as host wall time and as the time between two HIP events recorded on the null stream round the (blocking) calls — every
step ends in a stream synchronisation, so the two agree to the launch overhead. After (A) and (B) their results are compared byte for byte. Each step runs under a watchdog of its own: a step that
exceeds `--step-timeout` seconds ends the process with status 124 and nothing further is started.

    python3 tools/batch_preprocess_time.py --out build/batch_preprocess_time.json
"""
import argparse
import ctypes
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class HipEvents:
    def __init__(self):
        self.hip = None
        for name in ("libamdhip64.so", "libamdhip64.so.6", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
            try:
                self.hip = ctypes.CDLL(name)
                break
            except OSError:
                continue
        assert self.hip is not None, "libamdhip64.so not found"
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.hip.hipEventCreate(ctypes.byref(self.a)) == 0 and self.hip.hipEventCreate(ctypes.byref(self.b)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.a, None) == 0

    def stop_ms(self):
        ms = ctypes.c_float(0)
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def _expired(signum, frame):
    sys.stderr.write("batch_preprocess_time: a step exceeded its time limit; stopping\n")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "batch_preprocess_time.json"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--leaf", type=float, default=1.0)
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--only", default="", help="comma-separated subset of A,B,preprocess,align (default: all)")
    a = ap.parse_args()
    only = set(x for x in a.only.split(",") if x)
    from loc_lib_amd import api, synth

    rng = np.random.default_rng(1)
    distinct, inits = [], []
    for k in range(a.distinct):
        s = synth.make_scan(3 + k)
        x = np.zeros((len(s), 4), np.float32)
        x[:, :3] = s[:, :3]
        x[rng.integers(0, len(s), len(s) // 100), rng.integers(0, 3, len(s) // 100)] = np.nan
        distinct.append(x)
        inits.append(synth.make_pose(3 + k)[1])
    scans = [distinct[i % a.distinct] for i in range(a.scans)]
    poses = np.array([inits[i % a.distinct] for i in range(a.scans)])
    n_points = int(sum(len(s) for s in scans))
    res = dict(scans=a.scans, distinct=a.distinct, points=n_points, leaf=a.leaf, library=os.environ.get("LOCGPU_LIB") or "in-tree")

    ctx = api.Context(0)
    ev = HipEvents()
    marsh = api.MarshalledScans(scans)
    big = ctx.batch_empty(a.scans, max(len(s) for s in scans))
    big.upload_async(marsh)
    big.upload_wait()
    try:
        big.preprocess(a.leaf, out=ctx.batch_empty(a.scans, 1))
        raise SystemExit("a one-point dst cannot hold a filtered scan")
    except api.LocGpuError as e:
        need = e.counts
    M = int(need.max()) + 64
    res.update(filtered_points=int(need.sum()), filtered_max=int(need.max()), dst_points_per_scan=M)
    small_a, small_b = ctx.batch_empty(a.scans, M), ctx.batch_empty(a.scans, M)
    c_raw, c_fin, c_out = api.Cloud(ctx), api.Cloud(ctx), api.Cloud(ctx)

    def step_a():
        outs = []
        for s in scans:
            c_raw.upload(s, is_dense=False)
            c_raw.remove_nan(out=c_fin)
            c_fin.voxel_filter(a.leaf, out=c_out)
            outs.append(c_out.download())
        small_a.upload_async(outs)
        small_a.upload_wait()

    def step_b():
        big.upload_async(marsh)
        big.upload_wait()
        big.preprocess(a.leaf, out=small_b)

    if not only or "A" in only:
        timed("A_per_scan_filters_then_upload", step_a, ev, a.warm, a.reps, a.step_timeout, res)
    if not only or "B" in only:
        timed("B_upload_raw_then_preprocess", step_b, ev, a.warm, a.reps, a.step_timeout, res)
    if not only or {"A", "B"} <= only:  # faster and different is not faster: (B)'s batch holds (A)'s bytes, scan for scan
        res["outputs_equal"] = all(small_a.download_scan(k)[:, :3].tobytes() == small_b.download_scan(k)[:, :3].tobytes() for k in range(a.scans))
        print("outputs of (A) and (B) equal, all %d scans: %s" % (a.scans, res["outputs_equal"]), flush=True)
        assert res["outputs_equal"]
    if not only or "preprocess" in only:
        timed("preprocess_only_resident", lambda: big.preprocess(a.leaf, out=small_b), ev, a.warm, a.reps, a.step_timeout, res)
        ms = res["preprocess_only_resident"]["hip_event_ms_median"]
        res["preprocess_only_resident"]["slots_per_s"] = round(a.scans * big.max_points / (ms * 1e-3), 1)
    if not only or "align" in only:
        ctx.icp_set_target(synth.make_map(a.map_points))
        opts = api.icp_opts(method=api.P2PLANE)
        big.preprocess(a.leaf, out=small_b)
        timed("icp_align_batch_of_filtered", lambda: ctx.icp_align_batch(small_b, poses, opts), ev, a.warm, a.reps, a.step_timeout, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
