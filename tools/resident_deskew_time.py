#!/usr/bin/env python3
"""What the second pass of "ingest, align, derive the motion, compensate" costs: (A) sending the same blobs again through
locgpu_batch_upload_records_deskew against (B) locgpu_batch_deskew on the batch that is already resident, and what keeping the point
times costs the plain ingest: locgpu_batch_upload_records with locgpu_batch_keep_times on (T1) against off (T0). The four calls
alternate in ONE process, medians after warm-up.

Inputs: `--scans` scans of 64 x 1800 = 115 200 LAYOUT_VELODYNE records (32 B: xyz, intensity, float32 time = the column's firing time,
uint16 ring), one record per cell of a synth.make_range_image scan in ring-then-column order (`--distinct` different ones, repeated in
turn), a cell without a survivor as a NaN record; K = `--knots` knots per scan (the track of tools/range_deskew_time.py); the
reference time is the last column's. Reported: whole calls (host clock round the blocking call) and, with locgpu_profile_enable, the
kernels of each. Before any figure is written (B)'s batch is checked against (A)'s byte for byte, points, counts and rings. Each loop
runs under a watchdog: one that exceeds `--step-timeout` seconds ends the process with status 124 and nothing further is started.

    python3 tools/resident_deskew_time.py            # writes profiles/resident_deskew.json and profiles/resident_deskew.md
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
    sys.stderr.write("resident_deskew_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def med(xs):
    return round(float(np.median(xs)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_deskew"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--knots", type=int, default=3)
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
    cell_ring, cell_col = np.divmod(np.arange(model.cells), n_cols)
    blobs = []
    for k in range(a.distinct):
        raw, rings, cols = dref.survivors(model, synth.make_range_image(3 + k, model))
        xyz = np.full((model.cells, 3), np.nan, np.float32)  # a cell without a survivor: a record Conver drops
        xyz[rings.astype(np.int64) * n_cols + cols] = raw[:, :3]
        blobs.append(rref.pack(layout, xyz, col[cell_col].astype(np.float32), cell_ring, np.zeros(model.cells)))
    blobs = [blobs[i % a.distinct] for i in range(a.scans)]
    tracks = [make_track(a.knots, sweep, i % a.distinct) for i in range(a.scans)]
    kt, kp = np.stack([t for t, _ in tracks]), np.stack([p for _, p in tracks])
    rt = np.full(a.scans, col[-1])
    offs = np.zeros(a.scans)
    motion = dict(knot_times=kt, knot_poses=kp, ref_times=rt)

    ctx = api.Context(0)
    src, dst, ing, off = (ctx.batch_empty(a.scans, model.cells) for _ in range(4))
    src.keep_times()
    # correctness first: (B) leaves what (A) leaves
    counts = src.upload_records(layout, blobs)
    src.deskew(dst, offs, **motion)
    counts_a = ing.upload_records_deskew(layout, blobs, offs, kt, kp, rt)
    ok = counts.tolist() == counts_a.tolist()
    for s in sorted({0, a.scans // 2, a.scans - 1}):
        ok = ok and dst.download_scan(s).tobytes() == ing.download_scan(s).tobytes() and np.array_equal(dst.download_rings(s), ing.download_rings(s))
    print("the resident pass leaves the bytes of the deskewed ingest (points, counts, rings): %s" % ok, flush=True)
    assert ok
    points = int(counts.sum())
    rec_bytes = sum(len(b) for b in blobs)
    res = dict(scans=a.scans, distinct=a.distinct, records=a.scans * model.cells, points=points, record_bytes=rec_bytes, knots=a.knots, reps=a.reps,
               output_equals_deskewed_ingest=bool(ok))

    t = {k: [] for k in ("A_call", "A_copy", "A_kernels", "B_call", "B_check", "B_move", "T1_call", "T1_copy", "T1_kernels", "T0_call", "T0_copy", "T0_kernels")}
    ctx.profile_enable(True)
    signal.alarm(a.step_timeout)
    for it in range(a.warm + a.reps):  # alternating: whatever drifts, drifts under all
        t0 = time.perf_counter()
        ing.upload_records_deskew(layout, blobs, offs, kt, kp, rt)
        t1 = time.perf_counter()
        ra = ctx.records_ingest_times()
        src.deskew(dst, offs, **motion)
        t2 = time.perf_counter()
        rb = ctx.batch_deskew_times()
        src.upload_records(layout, blobs)
        t3 = time.perf_counter()
        r1 = ctx.records_ingest_times()
        off.upload_records(layout, blobs)
        t4 = time.perf_counter()
        r0 = ctx.records_ingest_times()
        if it >= a.warm:
            for name, call, (x, y) in (("A", t1 - t0, ra), ("T1", t3 - t2, r1), ("T0", t4 - t3, r0)):
                t[name + "_call"].append(1e3 * call)
                t[name + "_copy"].append(x)
                t[name + "_kernels"].append(y)
            t["B_call"].append(1e3 * (t2 - t1))
            t["B_check"].append(rb[0])
            t["B_move"].append(rb[1])
    signal.alarm(0)
    ctx.profile_enable(False)
    for k, v in t.items():
        res[k + "_ms"] = med(v)
    res["B_kernels_ms"] = round(res["B_check_ms"] + res["B_move_ms"], 3)
    # bytes of the pass: the check reads 8 B per point; the move reads 16 + 8 + 1 and writes 16 + 1 (dst is another batch: the ring byte too)
    res["B_pass_bytes"] = (8 + 25 + 17) * points
    res["B_pass_TBs"] = round(res["B_pass_bytes"] / (res["B_kernels_ms"] * 1e-3) / 1e12, 3)
    res["B_at_copy_rate_ms"] = round(res["B_pass_bytes"] / (COPY_TBS * 1e12) * 1e3, 3)
    res["A_over_B_call"] = round(res["A_call_ms"] / res["B_call_ms"], 2)
    res["keep_times_extra_call_ms"] = round(res["T1_call_ms"] - res["T0_call_ms"], 3)
    res["keep_times_extra_kernels_ms"] = round(res["T1_kernels_ms"] - res["T0_kernels_ms"], 3)
    res["times_resident_MB"] = round(8 * a.scans * model.cells / 1e6, 1)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# Compensating a resident batch against ingesting it a second time\n\n")
        f.write("`python tools/resident_deskew_time.py`: %d scans of %d LAYOUT_VELODYNE records (%d distinct, one record per cell of a 64 x 1800\n"
                "synth.make_range_image scan, %.1f MB of records, %d survivors), K = %d knots per scan, one process, the four calls alternating, medians of\n"
                "%d after %d warm-up rounds; whole calls by the host clock round the blocking call, the rest by HIP events (`locgpu_records_ingest_times`,\n"
                "`locgpu_batch_deskew_times`).\n\n" % (a.scans, model.cells, a.distinct, rec_bytes / 1e6, points, a.knots, a.reps, a.warm))
        f.write("**Status: measured.** The batch `locgpu_batch_deskew` leaves equals the one `locgpu_batch_upload_records_deskew` leaves byte for byte\n"
                "(points, counts, rings), checked before the timing.\n\n")
        f.write("| | (A) `upload_records_deskew` again | (B) `batch_deskew`, resident | (T1) `upload_records`, times kept | (T0) `upload_records` |\n|---|---|---|---|---|\n")
        f.write("| whole call | %.3f ms | %.3f ms | %.3f ms | %.3f ms |\n" % (res["A_call_ms"], res["B_call_ms"], res["T1_call_ms"], res["T0_call_ms"]))
        f.write("| copy stream (host staging included) | %.3f ms | none | %.3f ms | %.3f ms |\n" % (res["A_copy_ms"], res["T1_copy_ms"], res["T0_copy_ms"]))
        f.write("| kernels | %.3f ms | %.3f ms (check %.3f, move %.3f) | %.3f ms | %.3f ms |\n"
                % (res["A_kernels_ms"], res["B_kernels_ms"], res["B_check_ms"], res["B_move_ms"], res["T1_kernels_ms"], res["T0_kernels_ms"]))
        f.write("\n- The second pass: (A) %.3f ms against (B) %.3f ms per whole call, %.2f x. (B) sends %d knots per scan and nothing else over PCIe.\n"
                % (res["A_call_ms"], res["B_call_ms"], res["A_over_B_call"], a.knots))
        f.write("- (B)'s bytes: 8 B per point read by the check, 25 B read and 17 B written by the move = %.1f MB; at the float4 copy rate of\n"
                "  profiles/global_map.md (%.2f TB/s) that is %.3f ms; the two kernels take %.3f ms = %.3f TB/s nominal. (A)'s kernels, which also pick the\n"
                "  fields out of the records and compact, take %.3f ms.\n"
                % (res["B_pass_bytes"] / 1e6, COPY_TBS, res["B_at_copy_rate_ms"], res["B_kernels_ms"], res["B_pass_TBs"], res["A_kernels_ms"]))
        f.write("- Keeping the times costs the plain ingest %+.3f ms per whole call (%+.3f ms of kernels) and %.1f MB of HBM for this batch\n"
                "  (8 B per point slot).\n" % (res["keep_times_extra_call_ms"], res["keep_times_extra_kernels_ms"], res["times_resident_MB"]))
        f.write("- The move kernel is %.1f x its bytes at the copy rate: like the per-point deskew of the ingest (profiles/record_ingest.md) it is carried\n"
                "  by each lane's dependent FP64 chain (slerp, two rotation matrices, their product) at 4 waves per SIMD, not by memory. Counters: unmeasured.\n"
                % (res["B_move_ms"] / (42 * points / (COPY_TBS * 1e12) * 1e3)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
