#!/usr/bin/env python3
"""What motion compensation at decode costs on a whole batch: locgpu_batch_upload_ranges and locgpu_batch_upload_ranges_deskew of the
same images, alternating in ONE process, medians after warm-up.

Inputs: `--scans` scans of 64 x 1800 cells from synth.make_range_image (`--distinct` different ones, repeated in turn), min_range 4,
2 mm per count; column times uniform over a 0.1 s sweep; K = 11 knots per scan (a 100 Hz track over the sweep: 15 m/s forwards, a yaw
rate of 0.5 rad/s, translations near (100, -40, 2) m); the reference time is the last column's. Reported: both whole calls (host clock
round the blocking call), and with locgpu_profile_enable the copies, the matrix kernel (rd_pose_kernel) and the four decode kernels of
the deskewed call next to the plain call's two, and the ratio of the two decode passes. Before any figure is written, scan 0 of the
deskewed batch is checked against the numpy restatement (tests/range_deskew_ref.py) with the matrices downloaded from the device, byte
for byte. Each loop runs under a watchdog: one that exceeds `--step-timeout` seconds ends the process with status 124 and nothing
further is started.

    python3 tools/range_deskew_time.py            # writes profiles/range_deskew.json and profiles/range_deskew.md
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _expired(signum, frame):
    sys.stderr.write("range_deskew_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def med(xs):
    return round(float(np.median(xs)), 3)


def make_track(K, sweep, seed):
    """K knots over `sweep` seconds: 15 m/s along the heading, 0.5 rad/s of yaw, a start that differs per seed."""
    t = np.linspace(0.0, sweep, K)
    yaw = 0.3 * seed + 0.5 * t
    poses = np.zeros((K, 7))
    poses[:, 2], poses[:, 3] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
    poses[:, 4:] = np.array([100.0, -40.0, 2.0]) + np.stack([15.0 * t * np.cos(yaw[0]), 15.0 * t * np.sin(yaw[0]), 0.0 * t], 1)
    return t, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_deskew"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--knots", type=int, default=11)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    import range_deskew_ref as dref
    from loc_lib_amd import api, synth

    signal.signal(signal.SIGALRM, _expired)
    n_rings, n_cols, sweep = 64, 1800, 0.1
    model = api.SensorModel(n_rings, n_cols, 0.002, 4.0, *synth.sensor_tables(n_rings, n_cols))
    distinct = [synth.make_range_image(3 + k, model) for k in range(a.distinct)]
    images = [distinct[i % a.distinct] for i in range(a.scans)]
    col = np.linspace(0.0, sweep, n_cols)
    tracks = [make_track(a.knots, sweep, i % a.distinct) for i in range(a.scans)]
    kt, kp = np.stack([t for t, _ in tracks]), np.stack([p for _, p in tracks])
    rt = np.full(a.scans, col[-1])

    ctx = api.Context(0)
    sensor = api.Sensor(ctx, model)
    sensor.set_col_times(col)
    plain, desk = ctx.batch_empty(a.scans, model.cells), ctx.batch_empty(a.scans, model.cells)
    counts = desk.upload_ranges_deskew(sensor, images, kt, kp, rt)
    raw, rings, cols = dref.survivors(model, images[0])
    ok = desk.download_scan(0).tobytes() == dref.apply(raw, cols, ctx.range_deskew_matrices(0)).tobytes() and np.array_equal(desk.download_rings(0), rings)
    print("scan 0 of the deskewed batch equals the restatement byte for byte: %s" % ok, flush=True)
    assert ok
    points = int(counts.sum())
    res = dict(scans=a.scans, distinct=a.distinct, cells_per_scan=model.cells, points=points, knots=a.knots, reps=a.reps, output_equals_restatement=bool(ok),
               matrix_table_bytes=96 * a.scans * n_cols)

    t = dict(plain_call=[], plain_h2d=[], plain_decode=[], deskew_call=[], deskew_h2d=[], deskew_pose=[], deskew_decode=[])
    ctx.profile_enable(True)
    signal.alarm(a.step_timeout)
    for it in range(a.warm + a.reps):  # alternating: whatever drifts, drifts under both
        t0 = time.perf_counter()
        plain.upload_ranges(sensor, images)
        t1 = time.perf_counter()
        desk.upload_ranges_deskew(sensor, images, kt, kp, rt)
        t2 = time.perf_counter()
        p, d = ctx.range_ingest_times(), ctx.range_deskew_times()
        if it >= a.warm:
            t["plain_call"].append(1e3 * (t1 - t0))
            t["deskew_call"].append(1e3 * (t2 - t1))
            t["plain_h2d"].append(p[0])
            t["plain_decode"].append(p[1])
            t["deskew_h2d"].append(d[0])
            t["deskew_pose"].append(d[1])
            t["deskew_decode"].append(d[2])
    signal.alarm(0)
    ctx.profile_enable(False)
    for k, v in t.items():
        res[k + "_ms"] = med(v)
    res["decode_ratio"] = round(res["deskew_decode_ms"] / res["plain_decode_ms"], 3) if res["plain_decode_ms"] > 0 else None
    # the deskewed decode pass: 2 x 2 B per cell read, 96 B of matrix gathered and 17 B written per survivor
    res["deskew_decode_bytes"] = 4 * model.cells * a.scans + (96 + 17) * points
    res["deskew_decode_TBs"] = round(res["deskew_decode_bytes"] / (res["deskew_decode_ms"] * 1e-3) / 1e12, 3) if res["deskew_decode_ms"] > 0 else None

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# Motion compensation at decode next to the plain range-image ingest\n\n")
        f.write("`python tools/range_deskew_time.py`: %d scans of %d x %d cells (%d distinct, synth.make_range_image), %d points after Conver's rules,\n"
                "K = %d knots per scan, one process, the two calls alternating, medians of %d after %d warm-up rounds; whole calls by the host clock\n"
                "round the blocking call, the rest by HIP events (`locgpu_range_ingest_times`, `locgpu_range_deskew_times`).\n\n"
                % (a.scans, n_rings, n_cols, a.distinct, points, a.knots, a.reps, a.warm))
        f.write("**Status: measured.** Scan 0 of the deskewed batch equals the numpy restatement byte for byte, given the device's matrices.\n\n")
        f.write("| | `locgpu_batch_upload_ranges` | `locgpu_batch_upload_ranges_deskew` |\n|---|---|---|\n")
        f.write("| whole call | %.3f ms | %.3f ms |\n" % (res["plain_call_ms"], res["deskew_call_ms"]))
        f.write("| copies (copy stream, host staging included; deskewed: + %.1f KB of knots) | %.3f ms | %.3f ms |\n"
                % (8 * (8 * a.knots + 1) * a.scans / 1e3, res["plain_h2d_ms"], res["deskew_h2d_ms"]))
        f.write("| matrix kernel (`rd_pose_kernel`, %d x %d matrices, %.1f MB) | | %.3f ms |\n" % (a.scans, n_cols, res["matrix_table_bytes"] / 1e6, res["deskew_pose_ms"]))
        f.write("| decode pass (four kernels) | %.3f ms | %.3f ms = %.2f x the plain pass: %.1f MB at %s TB/s |\n"
                % (res["plain_decode_ms"], res["deskew_decode_ms"], res["decode_ratio"], res["deskew_decode_bytes"] / 1e6, res["deskew_decode_TBs"]))
        f.write("\nNotes. The deskewed pass's bytes count 2 x 2 B per cell read, 17 B per survivor written and the 96 B matrix each survivor's lane\n"
                "gathers; neighbouring survivors of a ring read neighbouring matrices, and survivors of one column in different rings read the same\n"
                "one, so how much of the gather reaches HBM was not measured; a nominal rate above the 6.29 TB/s float4 copy of\n"
                "profiles/global_map.md means that most of it was served by the caches.\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
