#!/usr/bin/env python3
"""What the target ingest of scan-to-scan odometry costs with the KD-trees built on the host and on the device, in one
process, on the workload of profiles/pairs.md: `--scans` consecutive synthetic scans filtered at `--leaf` by locgpu_batch_preprocess
into a resident batch, 255 pairs (scan i against scan i - 1), identity start, point-to-plane, the options' defaults.

  (B) locgpu_icp_set_target_forest_batch(batch) + locgpu_icp_align_pairs(batch, [-1, 0, 1, ...]): trees built on the host;
  (C) locgpu_icp_set_target_forest_device(batch) + the same locgpu_icp_align_pairs: trees built on the device.

and for ONE resident cloud of `--cloud` points (a keyframe local map): locgpu_icp_set_target_cloud against
locgpu_icp_set_target_cloud_device.

Before any timing: the forest's bytes after (B) and after (C) — read back through locgpu_debug_tree_read, pads and sentinel leaves
included — are compared, the report of (C) must say "device path", and the 256 poses and iteration counts of the two alignments must
be equal bit for bit; the single cloud's slots and leaf slots likewise. Then (B) and (C) alternate: `--warm` warm-up rounds, medians
of `--reps`, host wall time round blocking calls (every one ends in a stream synchronisation). LOCGPU_FOREST_TIMES=1 is set for the
process, so the library prints its own phases on stderr (host build | device buffers + H2D; the device kernel between two events);
stderr goes to a file during the timed rounds and the medians of those lines are reported too. Each step runs under a watchdog: a
step that exceeds `--step-timeout` seconds ends the process with status 124 and nothing further is started.

    python3 tools/forest_build_time.py --out build/forest_build_time.json
"""
import argparse
import json
import os
import re
import signal
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _expired(signum, frame):
    sys.stderr.write("forest_build_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def _stat(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3), reps=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "forest_build_time.json"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--first", type=int, default=3, help="id of the first scan of the circuit")
    ap.add_argument("--subsample", type=int, default=0, help="> 0: points kept of each raw scan (rehearsals)")
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--cloud", type=int, default=35000, help="points of the single cloud (a keyframe local map)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    os.environ["LOCGPU_FOREST_TIMES"] = "1"
    os.environ["LOCGPU_INGEST_TIMES"] = "1"
    from loc_lib_amd import api, synth

    signal.signal(signal.SIGALRM, _expired)
    signal.alarm(a.step_timeout)
    raw = []
    for k in range(a.scans):
        s = synth.make_scan(a.first + k, subsample=a.subsample or None)
        x = np.zeros((len(s), 4), np.float32)
        x[:, :3] = s[:, :3]
        raw.append(x)
    signal.alarm(0)
    res = dict(scans=a.scans, raw_points=int(sum(len(s) for s in raw)), leaf=a.leaf, library=os.environ.get("LOCGPU_LIB") or "in-tree")

    log = tempfile.NamedTemporaryFile(prefix="forest_build_time_", suffix=".stderr", delete=False)
    saved_err = os.dup(2)
    os.dup2(log.fileno(), 2)  # the library's phase lines, from here on
    try:
        ctx = api.Context(0)
        big = ctx.batch(raw)
        try:
            big.preprocess(a.leaf, out=ctx.batch_empty(a.scans, 1))
            raise SystemExit("a one-point dst cannot hold a filtered scan")
        except api.LocGpuError as e:
            need = e.counts
        small = ctx.batch_empty(a.scans, int(need.max()) + 64)
        big.preprocess(a.leaf, out=small)
        big.close()
        del raw
        res.update(filtered_points=int(need.sum()), filtered_max=int(need.max()), filtered_min=int(need.min()))
        print("filtered: %d points in %d scans (%d … %d)" % (res["filtered_points"], a.scans, res["filtered_min"], res["filtered_max"]), flush=True)

        opts = api.icp_opts(method=api.P2PLANE)
        target_of = np.arange(-1, a.scans - 1, dtype=np.int32)
        t = {}

        def clock(name, fn):
            t0 = time.perf_counter()
            out = fn()
            t.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))
            return out

        def step(tag, ingest):
            clock(tag + "_ingest", lambda: ingest(small))
            poses, stats = clock(tag + "_align_pairs", lambda: ctx.icp_align_pairs(small, target_of, None, opts))
            return poses, stats

        def bits(x):
            return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)

        # faster and different is not faster: the bytes and the poses first
        signal.alarm(a.step_timeout)
        pb, sb = step("B", ctx.icp_set_target_forest_batch)
        slots_b = ctx.debug_tree_read()[0]
        info_b = (ctx.icp_forest_info(), ctx.icp_target_info())
        pc, sc = step("C", ctx.icp_set_target_forest_device)
        slots_c = ctx.debug_tree_read()[0]
        info_c = (ctx.icp_forest_info(), ctx.icp_target_info())
        build = ctx.icp_device_build_info()
        signal.alarm(0)
        res.update(forest_slots=int(len(slots_c)), forest_bytes_equal=bool(slots_b.shape == slots_c.shape and np.array_equal(slots_b, slots_c)),
                   infos_equal=bool(info_b == info_c), device_path=bool(build["path"] == api.BUILD_PATH_DEVICE), build_info=build,
                   poses_equal=bool(np.array_equal(bits(pb), bits(pc))), stats_equal=bool(sb == sc),
                   iterations_mean=float(np.mean([s["iterations"] for s in sc[1:]])))
        print("forest: %d slots, bytes equal %s, infos equal %s, device path %s; poses equal %s, stats equal %s" %
              (res["forest_slots"], res["forest_bytes_equal"], res["infos_equal"], res["device_path"], res["poses_equal"], res["stats_equal"]), flush=True)
        if not (res["forest_bytes_equal"] and res["infos_equal"] and res["device_path"] and res["poses_equal"] and res["stats_equal"]):
            raise SystemExit("the device build is not the host build: nothing is timed")

        m = synth.make_local_map(a.cloud, a.first, half=30.0)
        xyzi = np.zeros((len(m), 4), np.float32)
        xyzi[:, :3] = m[:, :3]
        cctx = api.Context(0)
        cloud = api.Cloud(cctx, xyzi)
        signal.alarm(a.step_timeout)
        cctx.icp_set_target_cloud(cloud)
        one_b = cctx.debug_tree_read()
        cctx.icp_set_target_cloud_device(cloud)
        one_c = cctx.debug_tree_read()
        cbuild = cctx.icp_device_build_info()
        signal.alarm(0)
        res.update(cloud_points=int(len(m)), cloud_bytes_equal=bool(np.array_equal(one_b[0], one_c[0]) and np.array_equal(one_b[1], one_c[1])),
                   cloud_device_path=bool(cbuild["path"] == api.BUILD_PATH_DEVICE), cloud_build_info=cbuild)
        print("single cloud: %d points, bytes equal %s, device path %s" % (res["cloud_points"], res["cloud_bytes_equal"], res["cloud_device_path"]), flush=True)
        if not (res["cloud_bytes_equal"] and res["cloud_device_path"]):
            raise SystemExit("the single cloud's device build is not the host build: nothing is timed")

        mark = 0
        for r in range(a.warm + a.reps):
            signal.alarm(a.step_timeout)
            if r == a.warm:
                t.clear()
                os.fsync(2)
                mark = os.path.getsize(log.name)
            clock("B_whole", lambda: step("B", ctx.icp_set_target_forest_batch))
            clock("C_whole", lambda: step("C", ctx.icp_set_target_forest_device))
            clock("cloud_host", lambda: cctx.icp_set_target_cloud(cloud))
            clock("cloud_device", lambda: cctx.icp_set_target_cloud_device(cloud))
            signal.alarm(0)
            print("round %d done" % r, flush=True)
    finally:
        os.dup2(saved_err, 2)
        os.close(saved_err)
    # the library's own lines of the timed rounds
    with open(log.name) as f:
        f.seek(mark)
        lines = f.read().splitlines()
    os.unlink(log.name)
    phases = {}
    for line in lines:
        for pat, name in ((r"\[locgpu forest ingest\] host build ([\d.]+) ms", "B_lib_host_build"), (r"\[locgpu forest ingest\] device buffers \+ H2D ([\d.]+) ms", "B_lib_buffers_h2d"),
                          (r"\[locgpu forest device\] forest_build_kernel ([\d.]+) ms \((\d+) trees", "kernel"), (r"\[locgpu ingest\] host build ([\d.]+) ms", "cloud_lib_host_build"),
                          (r"\[locgpu ingest\] device buffers \+ H2D ([\d.]+) ms", "cloud_lib_buffers_h2d")):
            mm = re.search(pat, line)
            if mm:
                key = name if name != "kernel" else ("C_kernel_forest" if int(mm.group(2)) > 1 else "cloud_kernel")
                phases.setdefault(key, []).append(float(mm.group(1)))
    for name, v in list(t.items()) + list(phases.items()):
        res[name] = _stat(v)
        print("%-28s %9.3f ms (min %9.3f, max %9.3f, %d)" % (name, res[name]["median"], res[name]["min"], res[name]["max"], res[name]["reps"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
