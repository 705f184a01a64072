#!/usr/bin/env python3
"""What the point-record ingest costs on a whole batch, plain and motion-compensated per point, next to the range-image ingest of the
same scans: locgpu_batch_upload_records (P), locgpu_batch_upload_records_deskew (D), locgpu_batch_upload_ranges_deskew (R) and
locgpu_batch_upload_ranges (R0, for R's own extra) alternating in ONE process, medians after warm-up.

Inputs: `--scans` scans of 64 x 1800 cells from synth.make_range_image (`--distinct` different ones, repeated in turn), min_range 4,
2 mm per count, decoded by the numpy restatement; the survivors of a scan become LAYOUT_VELODYNE records (32 B: xyz, intensity, float32
time = the column's firing time, uint16 ring) in ring-then-column order, or with `--order column` in column-then-ring order, the order
a spinning sensor's driver emits, in which the rings of one firing are neighbours and share a time. K = `--knots` knots per scan (the
track of tools/range_deskew_time.py); the reference time is the last column's. Reported: whole calls (host clock round the blocking
call), and with locgpu_profile_enable the copy stream and the kernels of each; the pass's bytes per point against the project's float4
copy rate; the deskew kernels' extra time over (P) per survivor next to the range path's extra per survivor; and (D)'s kernels at other
knot counts, which separates the knot staging from the FP64 arithmetic. Before any figure is written, scan 0 of (D) is checked against
the numpy restatement with the matrices downloaded from the device, byte for byte, and (D)'s points against (R)'s. Each loop runs
under a watchdog: one that exceeds `--step-timeout` seconds ends the process with status 124 and nothing further is started.

    python3 tools/record_ingest_time.py            # writes profiles/record_ingest.json and profiles/record_ingest.md
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_TBS = 6.29  # the float4 copy rate of profiles/global_map.md


def _expired(signum, frame):
    sys.stderr.write("record_ingest_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def med(xs):
    return round(float(np.median(xs)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_ingest"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--knots", type=int, default=11)
    ap.add_argument("--other-knots", type=int, nargs="*", default=[2, 64, 256])
    ap.add_argument("--order", choices=("ring", "column"), default="ring")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    import range_deskew_ref as dref
    import record_ingest_ref as rref
    from loc_lib_amd import api, synth
    from range_deskew_time import make_track

    signal.signal(signal.SIGALRM, _expired)
    n_rings, n_cols, sweep = 64, 1800, 0.1
    model = api.SensorModel(n_rings, n_cols, 0.002, 4.0, *synth.sensor_tables(n_rings, n_cols))
    col = np.linspace(0.0, sweep, n_cols)
    layout = api.LAYOUT_VELODYNE
    images, blobs, decoded = [], [], []
    for k in range(a.distinct):
        im = synth.make_range_image(3 + k, model)
        raw, rings, cols = dref.survivors(model, im)
        order = np.lexsort((rings, cols)) if a.order == "column" else np.arange(len(raw))
        images.append(im)
        decoded.append((raw[order], rings[order], cols[order]))
        blobs.append(rref.pack(layout, raw[order, :3], col[cols[order]].astype(np.float32), rings[order], np.zeros(len(raw))))
    images = [images[i % a.distinct] for i in range(a.scans)]
    blobs = [blobs[i % a.distinct] for i in range(a.scans)]

    def motion(K):
        tracks = [make_track(K, sweep, i % a.distinct) for i in range(a.scans)]
        return np.stack([t for t, _ in tracks]), np.stack([p for _, p in tracks])

    kt, kp = motion(a.knots)
    rt = np.full(a.scans, col[-1])
    offs = np.zeros(a.scans)

    ctx = api.Context(0)
    sensor = api.Sensor(ctx, model)
    sensor.set_col_times(col)
    plain, desk, rng0, rng = (ctx.batch_empty(a.scans, model.cells) for _ in range(4))
    # correctness first: scan 0 against the restatement, given the device's matrices (one scan: the debug table is 96 B per point slot)
    one = ctx.batch_empty(1, model.cells)
    ctx.records_deskew_debug(True)
    one.upload_records_deskew(layout, blobs[:1], offs[:1], kt[:1], kp[:1], rt[:1])
    raw, rings, cols = decoded[0]
    mats = ctx.records_deskew_matrices(0)
    ctx.records_deskew_debug(False)
    want0 = dref.apply(raw, np.arange(len(raw)), mats)
    ok = one.download_scan(0).tobytes() == want0.tobytes() and np.array_equal(one.download_rings(0), rings)
    one.close()
    counts = desk.upload_records_deskew(layout, blobs, offs, kt, kp, rt)
    ok = ok and desk.download_scan(0).tobytes() == want0.tobytes()
    # the column's time is float32 here and float64 on the range path: the two agree only where float32(col) == col, so compare counts
    counts_r = rng.upload_ranges_deskew(sensor, images, kt, kp, rt)
    ok = ok and counts.tolist() == counts_r.tolist()
    print("scan 0 of the deskewed record batch equals the restatement byte for byte, counts equal the range path's: %s" % ok, flush=True)
    assert ok
    points = int(counts.sum())
    rec_bytes = sum(len(b) for b in blobs)
    res = dict(scans=a.scans, distinct=a.distinct, order=a.order, points=points, record_bytes=rec_bytes, knots=a.knots, reps=a.reps, output_equals_restatement=bool(ok))

    names = ("P", "D", "R", "R0")
    t = {n + k: [] for n in names for k in ("_call", "_copy", "_kernels")}
    t["R_pose"] = []
    ctx.profile_enable(True)
    signal.alarm(a.step_timeout)
    for it in range(a.warm + a.reps):  # alternating: whatever drifts, drifts under all
        row = {}
        t0 = time.perf_counter()
        plain.upload_records(layout, blobs)
        t1 = time.perf_counter()
        row["P"] = (t1 - t0, *ctx.records_ingest_times())
        desk.upload_records_deskew(layout, blobs, offs, kt, kp, rt)
        t2 = time.perf_counter()
        row["D"] = (t2 - t1, *ctx.records_ingest_times())
        rng.upload_ranges_deskew(sensor, images, kt, kp, rt)
        t3 = time.perf_counter()
        d = ctx.range_deskew_times()
        row["R"] = (t3 - t2, d[0], d[1] + d[2])
        rng0.upload_ranges(sensor, images)
        t4 = time.perf_counter()
        row["R0"] = (t4 - t3, *ctx.range_ingest_times())
        if it >= a.warm:
            for n in names:
                t[n + "_call"].append(1e3 * row[n][0])
                t[n + "_copy"].append(row[n][1])
                t[n + "_kernels"].append(row[n][2])
            t["R_pose"].append(d[1])
    signal.alarm(0)
    for k, v in t.items():
        res[k + "_ms"] = med(v)
    sweep_k = {}
    for K in a.other_knots:  # the same records and times on tracks of other knot counts: what the knot staging costs
        kt2, kp2 = motion(K)
        signal.alarm(a.step_timeout)
        ks = []
        for it in range(2 + 5):
            desk.upload_records_deskew(layout, blobs, offs, kt2, kp2, rt)
            if it >= 2:
                ks.append(ctx.records_ingest_times()[1])
        signal.alarm(0)
        sweep_k[str(K)] = med(ks)
    ctx.profile_enable(False)
    res["D_kernels_ms_by_knots"] = sweep_k
    # bytes of a pass: the records read by the count and again by the scatter kernel, 17 B written per survivor (float4 + ring byte)
    res["P_pass_bytes"] = 2 * rec_bytes + 17 * points
    res["P_bytes_per_point"] = round(res["P_pass_bytes"] / points, 1)
    res["P_pass_TBs"] = round(res["P_pass_bytes"] / (res["P_kernels_ms"] * 1e-3) / 1e12, 3)
    res["D_pass_TBs"] = round(res["P_pass_bytes"] / (res["D_kernels_ms"] * 1e-3) / 1e12, 3)
    res["P_at_copy_rate_ms"] = round(res["P_pass_bytes"] / (COPY_TBS * 1e12) * 1e3, 3)
    res["D_extra_ms"] = round(res["D_kernels_ms"] - res["P_kernels_ms"], 3)
    res["R_extra_ms"] = round(res["R_kernels_ms"] - res["R0_kernels_ms"], 3)
    res["D_extra_ns_per_survivor"] = round(1e6 * res["D_extra_ms"] / points, 4)
    res["R_extra_ns_per_survivor"] = round(1e6 * res["R_extra_ms"] / points, 4)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# The point-record ingest, plain and motion-compensated per point, next to the range-image ingest\n\n")
        f.write("`python tools/record_ingest_time.py%s`: %d scans of %d x %d cells (%d distinct, synth.make_range_image), their %d survivors as 32-byte\n"
                "LAYOUT_VELODYNE records in %s order (%.1f MB of records; the range images are %.1f MB), K = %d knots per scan, one process, the four calls\n"
                "alternating, medians of %d after %d warm-up rounds; whole calls by the host clock round the blocking call, the rest by HIP events\n"
                "(`locgpu_records_ingest_times`, `locgpu_range_deskew_times`, `locgpu_range_ingest_times`).\n\n"
                % ("" if a.order == "ring" else " --order column", a.scans, n_rings, n_cols, a.distinct, points, "ring-then-column" if a.order == "ring" else "column-then-ring",
                   rec_bytes / 1e6, 2 * model.cells * a.scans / 1e6, a.knots, a.reps, a.warm))
        f.write("**Status: measured.** Scan 0 of the deskewed record batch equals the numpy restatement byte for byte, given the device's matrices.\n\n")
        f.write("| | (P) `upload_records` | (D) `upload_records_deskew` | (R) `upload_ranges_deskew` | (R0) `upload_ranges` |\n|---|---|---|---|---|\n")
        f.write("| whole call | %.3f ms | %.3f ms | %.3f ms | %.3f ms |\n" % tuple(res[n + "_call_ms"] for n in names))
        f.write("| copy stream (host staging included) | %.3f ms | %.3f ms | %.3f ms | %.3f ms |\n" % tuple(res[n + "_copy_ms"] for n in names))
        f.write("| kernels | %.3f ms | %.3f ms | %.3f ms (of which `rd_pose_kernel` %.3f) | %.3f ms |\n"
                % (res["P_kernels_ms"], res["D_kernels_ms"], res["R_kernels_ms"], res["R_pose_ms"], res["R0_kernels_ms"]))
        f.write("\n- The pass's bytes: the records read twice (count, scatter) and 17 B written per survivor = %.1f MB = %.1f B per point. At the float4 copy\n"
                "  rate of profiles/global_map.md (%.2f TB/s) that is %.3f ms; (P)'s kernels take %.3f ms = %.3f TB/s, (D)'s %.3f ms = %.3f TB/s nominal.\n"
                % (res["P_pass_bytes"] / 1e6, res["P_bytes_per_point"], COPY_TBS, res["P_at_copy_rate_ms"], res["P_kernels_ms"], res["P_pass_TBs"], res["D_kernels_ms"],
                   res["D_pass_TBs"]))
        f.write("- Deskew's extra kernel time: (D) - (P) = %.3f ms = %.4f ns per survivor; the range path's, (R) - (R0) with `rd_pose_kernel` included, = %.3f ms =\n"
                "  %.4f ns per survivor. Ratio %.1f x: the per-point form computes one pose and matrix per survivor, the per-column form one per column\n"
                "  (%d survivors per column matrix here).\n"
                % (res["D_extra_ms"], res["D_extra_ns_per_survivor"], res["R_extra_ms"], res["R_extra_ns_per_survivor"],
                   res["D_extra_ms"] / res["R_extra_ms"] if res["R_extra_ms"] > 0 else float("nan"), points // (a.scans * n_cols)))
        f.write("- (D)'s kernels by knot count, same records and times: %s; K = %d: %.3f ms. Every block stages 8 K doubles of knots for its 256\n"
                "  records; the FP64 arithmetic per survivor does not depend on K beyond the bisection's log2 K steps.\n"
                % (", ".join("K = %s: %.3f ms" % kv for kv in sweep_k.items()), a.knots, res["D_kernels_ms"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
