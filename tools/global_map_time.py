#!/usr/bin/env python3
"""What Lio::GetGlobalMap (lio.cpp:550-580: transform every keyframe, join, ONE voxel filter) costs on resident keyframes, two ways, in
one process on one GPU:

  (A) the per-keyframe composition through the single-cloud entry points: per keyframe locgpu_cloud_transform into a temporary and
      locgpu_cloud_append to the sum, then locgpu_cloud_voxel_filter — what the library offered before locgpu_clouds_merge;
  (B) one locgpu_clouds_merge.

Both are driven through the raw ctypes functions with the arguments marshalled beforehand (the cost of one such call is measured and
reported), on the same clouds, alternating (A), (B), (A) without its filter, (B) with leaf 0 (the transform-and-join launch alone:
table copy + launch + synchronisation) and the filter alone on the joined cloud, `--reps` times after `--warm` warm-up rounds; every
figure is the median (min … max) of the host wall time of blocking calls. After the rounds the two maps are compared byte for byte.

Workloads: (i) 256 keyframes of raw 115 200-point scans (what lio.cpp:254,275 save) — bandwidth-bound; (ii) 4096 keyframes of 9 000
points — launch-bound. Keyframes are `--distinct` synthetic scans in turn under their true poses, each lap of them shifted by 40 m.
Each workload runs under a watchdog: one that exceeds `--step-timeout` seconds ends the process with status 124.

    python3 tools/global_map_time.py --out build/global_map_time.json
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

WORKLOADS = {"i": dict(keyframes=256, points=None), "ii": dict(keyframes=4096, points=9000)}


def _expired(signum, frame):
    sys.stderr.write("global_map_time: a workload exceeded its time limit; stopping\n")
    os._exit(124)


def stats(xs):
    return dict(median_ms=round(float(np.median(xs)), 3), min_ms=round(min(xs), 3), max_ms=round(max(xs), 3), reps=len(xs))


def run(api, synth, name, n_kf, points, a, res):
    L = api.lib()
    ctx = api.Context(0)
    scans, true_poses = [], []
    for k in range(a.distinct):
        s = synth.make_scan(3 + k, subsample=points) if points else synth.make_scan(3 + k)
        x = np.zeros((len(s), 4), np.float32)
        x[:, :3] = s[:, :3]
        x[:, 3] = np.arange(len(s), dtype=np.float32) % 255.0
        scans.append(x)
        true_poses.append(synth.make_pose(3 + k)[0])
    poses = np.array([true_poses[i % a.distinct] for i in range(n_kf)])
    poses[:, 5] += 40.0 * (np.arange(n_kf) // a.distinct)
    clouds = [api.Cloud(ctx, scans[i % a.distinct]) for i in range(n_kf)]
    total = int(sum(len(scans[i % a.distinct]) for i in range(n_kf)))
    handles = (ctypes.c_void_p * n_kf)(*[c._h for c in clouds])
    pose_ptr = [poses[i].ctypes.data for i in range(n_kf)]
    acc, tmp, joined, out_a, out_b, out_f = (api.Cloud(ctx) for _ in range(6))
    empty = np.zeros((1, 4), np.float32)
    pt = ctypes.c_int(0)
    leaf = ctypes.c_float(a.leaf)

    def ok(rc):
        if rc != 0:
            raise api.LocGpuError(rc, L.locgpu_last_error(ctx._h).decode())

    def a_join():
        ok(L.locgpu_cloud_upload(acc._h, empty.ctypes.data, 0, 16, 12, 1))  # acc = a fresh cloud (its storage is kept)
        for i in range(n_kf):
            ok(L.locgpu_cloud_transform(handles[i], pose_ptr[i], tmp._h))
            ok(L.locgpu_cloud_append(acc._h, tmp._h))
        # the appends are only enqueued: the join has run when the stream is idle (the filter's read-back, or ctx_sync)

    def a_whole():
        a_join()
        ok(L.locgpu_cloud_voxel_filter(acc._h, leaf, out_a._h, ctypes.byref(pt)))

    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))

    def ctx_sync():
        assert hip.hipDeviceSynchronize() == 0

    def a_join_blocking():
        a_join()
        ctx_sync()

    def b_whole():
        ok(L.locgpu_clouds_merge(ctx._h, handles, poses.ctypes.data, n_kf, leaf, out_b._h, ctypes.byref(pt)))

    def b_join():
        ok(L.locgpu_clouds_merge(ctx._h, handles, poses.ctypes.data, n_kf, ctypes.c_float(0.0), joined._h, ctypes.byref(pt)))

    def filter_only():
        ok(L.locgpu_cloud_voxel_filter(joined._h, leaf, out_f._h, ctypes.byref(pt)))

    steps = [("A_whole", a_whole), ("B_whole", b_whole), ("A_join", a_join_blocking), ("B_join", b_join), ("filter_only", filter_only)]
    times = {k: [] for k, _ in steps}
    signal.signal(signal.SIGALRM, _expired)
    signal.alarm(a.step_timeout)
    for rep in range(a.warm + a.reps):
        for key, fn in steps:
            ctx_sync()
            t0 = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t0)
            if rep >= a.warm:
                times[key].append(dt)
    # one ctypes call that does nothing on the device: what (A)'s 2 n calls cost before they reach the library
    n_probe = 20000
    cnt = ctypes.c_size_t(0)
    t0 = time.perf_counter()
    for _ in range(n_probe):
        L.locgpu_cloud_info(acc._h, ctypes.byref(cnt), None)
    call_us = 1e6 * (time.perf_counter() - t0) / n_probe
    a_whole()
    b_whole()
    equal = out_a.download().tobytes() == out_b.download().tobytes() and out_a.info == out_b.info
    signal.alarm(0)
    r = dict(keyframes=n_kf, points=total, leaf=a.leaf, map_points=len(out_b), ctypes_call_us=round(call_us, 2), outputs_equal=bool(equal))
    for key, _ in steps:
        r[key] = stats(times[key])
    join_s = r["B_join"]["median_ms"] * 1e-3
    r["B_join"]["bytes"] = 32 * total
    r["B_join"]["TB_per_s_of_the_call"] = round(32 * total / join_s / 1e12, 3)
    res[name] = r
    print("workload (%s): %d keyframes, %d points, leaf %.2f -> %d map points; outputs of (A) and (B) equal: %s; one ctypes call %.2f us"
          % (name, n_kf, total, a.leaf, r["map_points"], equal, call_us))
    for key, _ in steps:
        print("  %-12s %9.3f ms  (%9.3f ... %9.3f)" % (key, r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"]))
    print("  B_join moves %d B: %.3f TB/s over the whole call (6.29 TB/s: a float4 copy)" % (32 * total, r["B_join"]["TB_per_s_of_the_call"]), flush=True)
    assert equal
    for c in clouds + [acc, tmp, joined, out_a, out_b, out_f]:
        c.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "global_map_time.json"))
    ap.add_argument("--workloads", default="i,ii")
    ap.add_argument("--keyframes", type=int, default=0, help="override the workload's number of keyframes (rehearsals)")
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=400)
    a = ap.parse_args()
    from loc_lib_amd import api, synth

    res = dict(library=os.environ.get("LOCGPU_LIB") or "in-tree")
    for name in a.workloads.split(","):
        w = WORKLOADS[name]
        run(api, synth, name, a.keyframes or w["keyframes"], w["points"], a, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
