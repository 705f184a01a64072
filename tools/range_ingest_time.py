#!/usr/bin/env python3
"""What the range-image ingest buys on a whole batch, measured two ways in ONE process, alternating, medians after warm-up:

  (A) the float path: locgpu_batch_upload_async + locgpu_batch_upload_wait of the decoded float clouds (16 B per point over PCIe),
      then locgpu_batch_preprocess;
  (C) locgpu_batch_upload_ranges of the range images (2 B per cell), then the same preprocess.

Inputs: `--scans` scans of 64 x 1800 cells from synth.make_range_image (`--distinct` different ones, repeated in turn), min_range 4,
2 mm per count, leaf 1.0. The float clouds of (A) are the numpy restatement's decode of the same images (tests/range_image_ref.py), so
both paths must leave the same bytes in every filtered scan — checked before any figure is written. Reported: both totals; the H2D
time and bytes of each ((A): the upload alone; (C): the copy stream's time with locgpu_profile_enable, host staging included); the
decode pass alone and its bytes/s; and the LOAM pipeline's share — locgpu_batch_loam_extract_resident against
locgpu_batch_loam_extract with host ring arrays. Each step runs under a watchdog: a step that exceeds `--step-timeout` seconds ends
the process with status 124 and nothing further is started.

    python3 tools/range_ingest_time.py            # writes profiles/range_ingest.json and profiles/range_ingest.md
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

FLOAT4_COPY_TBS = 6.29  # profiles/global_map.md: what a float4 copy reaches on this machine


def _expired(signum, frame):
    sys.stderr.write("range_ingest_time: a step exceeded its time limit; stopping\n")
    os._exit(124)


def med(xs):
    return round(float(np.median(xs)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_ingest"))
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    import range_image_ref as ref
    from loc_lib_amd import api, synth

    signal.signal(signal.SIGALRM, _expired)
    n_rings, n_cols = 64, 1800
    model = api.SensorModel(n_rings, n_cols, 0.002, 4.0, *synth.sensor_tables(n_rings, n_cols))
    distinct = [synth.make_range_image(3 + k, model) for k in range(a.distinct)]
    decoded = [ref.decode(model, im) for im in distinct]
    images = [distinct[i % a.distinct] for i in range(a.scans)]
    clouds = [decoded[i % a.distinct][0] for i in range(a.scans)]
    rings = [decoded[i % a.distinct][1] for i in range(a.scans)]
    points = int(sum(len(c) for c in clouds))
    res = dict(scans=a.scans, distinct=a.distinct, cells_per_scan=model.cells, points=points, leaf=a.leaf, reps=a.reps,
               bytes_h2d_A=16 * points, bytes_h2d_C=2 * model.cells * a.scans)

    ctx = api.Context(0)
    sensor = api.Sensor(ctx, model)
    marsh = api.MarshalledScans(clouds)
    raw_a, raw_c = ctx.batch_empty(a.scans, model.cells), ctx.batch_empty(a.scans, model.cells)
    raw_c.upload_ranges(sensor, images)
    try:
        raw_c.preprocess(a.leaf, out=ctx.batch_empty(a.scans, 1))
        raise SystemExit("a one-point dst cannot hold a filtered scan")
    except api.LocGpuError as e:
        M = int(e.counts.max()) + 64
    flt_a, flt_c = ctx.batch_empty(a.scans, M), ctx.batch_empty(a.scans, M)

    t = dict(A_total=[], A_h2d=[], C_total=[], C_upload_ranges=[], C_h2d=[], C_decode=[])
    ctx.profile_enable(True)
    signal.alarm(a.step_timeout)
    for it in range(a.warm + a.reps):  # alternating: whatever drifts, drifts under both
        t0 = time.perf_counter()
        raw_a.upload_async(marsh)
        raw_a.upload_wait()
        # upload_wait returns when the copies are ENQUEUED; the preprocess waits for them — time them with it, and alone below
        raw_a.preprocess(a.leaf, out=flt_a)
        t1 = time.perf_counter()
        raw_c.upload_ranges(sensor, images)
        t2 = time.perf_counter()
        raw_c.preprocess(a.leaf, out=flt_c)
        t3 = time.perf_counter()
        h2d, dec = ctx.range_ingest_times()
        raw_a.upload_async(marsh)
        raw_a.upload_wait()
        raw_a.download_scan(0)  # ordered behind the upload and blocking: the copies have landed
        t4 = time.perf_counter()
        if it >= a.warm:
            t["A_total"].append(1e3 * (t1 - t0))
            t["C_total"].append(1e3 * (t3 - t1))
            t["C_upload_ranges"].append(1e3 * (t2 - t1))
            t["C_h2d"].append(h2d)
            t["C_decode"].append(dec)
            t["A_h2d"].append(1e3 * (t4 - t3))
    signal.alarm(0)
    ctx.profile_enable(False)
    raw_a.preprocess(a.leaf, out=flt_a)
    raw_c.preprocess(a.leaf, out=flt_c)
    res["outputs_equal"] = all(flt_a.download_scan(k).tobytes() == flt_c.download_scan(k).tobytes() for k in range(a.scans))
    print("filtered scans of (A) and (C) equal, all %d: %s" % (a.scans, res["outputs_equal"]), flush=True)
    assert res["outputs_equal"]
    for k, v in t.items():
        res[k + "_ms"] = med(v)
    # the decode pass: 2 x 2 B per cell read, 17 B per survivor written
    dec_bytes = 4 * model.cells * a.scans + 17 * points
    res["decode_bytes"] = dec_bytes
    res["decode_TBs"] = round(dec_bytes / (res["C_decode_ms"] * 1e-3) / 1e12, 3) if res["C_decode_ms"] > 0 else None
    res["decode_vs_float4_copy"] = round(res["decode_TBs"] / FLOAT4_COPY_TBS, 3) if res["decode_TBs"] else None
    res["A_h2d_GBs"] = round(res["bytes_h2d_A"] / (res["A_h2d_ms"] * 1e-3) / 1e9, 2)
    res["C_h2d_GBs"] = round(res["bytes_h2d_C"] / (res["C_h2d_ms"] * 1e-3) / 1e9, 2) if res["C_h2d_ms"] > 0 else None

    # the LOAM pipeline's share: the picker with resident rings against the picker with host ring arrays (their pack + 1 B per point H2D)
    num_scan = n_rings
    loam_scans = min(a.scans, 65535 // num_scan)
    lr = ctx.batch_empty(loam_scans, model.cells)
    edge, surf = ctx.batch_empty(loam_scans, num_scan * 6 * 20), ctx.batch_empty(loam_scans, model.cells)
    lr.upload_ranges(sensor, images[:loam_scans])
    th, tr = [], []
    signal.alarm(a.step_timeout)
    for it in range(a.warm + a.reps):
        t0 = time.perf_counter()
        ne_h, ns_h, _ = lr.loam_extract(rings[:loam_scans], num_scan, edge, surf)
        t1 = time.perf_counter()
        ne_r, ns_r, _ = lr.loam_extract_resident(num_scan, edge, surf)
        t2 = time.perf_counter()
        assert ne_h.tolist() == ne_r.tolist() and ns_h.tolist() == ns_r.tolist()
        if it >= a.warm:
            th.append(1e3 * (t1 - t0))
            tr.append(1e3 * (t2 - t1))
    signal.alarm(0)
    res.update(loam_scans=loam_scans, loam_extract_host_rings_ms=med(th), loam_extract_resident_ms=med(tr))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# Range-image ingest next to the float upload\n\n")
        f.write("`python tools/range_ingest_time.py`: %d scans of %d x %d cells (%d distinct, synth.make_range_image), %d points after Conver's rules,\n"
                "leaf %.1f, one process, the two paths alternating, medians of %d after %d warm-up rounds, host clock round blocking calls.\n\n"
                % (a.scans, n_rings, n_cols, a.distinct, points, a.leaf, a.reps, a.warm))
        f.write("**Status: measured.** The filtered scans of (A) and (C) hold the same bytes in all %d scans.\n\n" % a.scans)
        f.write("| | (A) float clouds | (C) range images |\n|---|---|---|\n")
        f.write("| upload + `locgpu_batch_preprocess` | %.3f ms | %.3f ms |\n" % (res["A_total_ms"], res["C_total_ms"]))
        f.write("| bytes over PCIe | %.1f MB | %.1f MB |\n" % (res["bytes_h2d_A"] / 1e6, res["bytes_h2d_C"] / 1e6))
        f.write("| H2D (A: upload alone until landed; C: copy stream, host staging included) | %.3f ms, %.1f GB/s | %.3f ms, %s GB/s |\n"
                % (res["A_h2d_ms"], res["A_h2d_GBs"], res["C_h2d_ms"], res["C_h2d_GBs"]))
        f.write("| `locgpu_batch_upload_ranges`, whole call | | %.3f ms |\n" % res["C_upload_ranges_ms"])
        f.write("| decode pass alone (four kernels, HIP events) | | %.3f ms: %.1f MB at %s TB/s = %s of the %.2f TB/s float4 copy of profiles/global_map.md |\n"
                % (res["C_decode_ms"], dec_bytes / 1e6, res["decode_TBs"], res["decode_vs_float4_copy"], FLOAT4_COPY_TBS))
        f.write("\nLOAM picker on %d scans, %d rings: `locgpu_batch_loam_extract` with host ring arrays %.3f ms, `locgpu_batch_loam_extract_resident` %.3f ms.\n"
                % (loam_scans, num_scan, res["loam_extract_host_rings_ms"], res["loam_extract_resident_ms"]))
        f.write("\nNotes. (A)'s H2D row is the upload followed by a blocking read-back of one scan (1.8 MB), which is what orders the host behind\n"
                "the copies. The decode figure counts 2 x 2 B per cell read (the image is decoded in the count and in the scatter kernel) and 17 B\n"
                "per survivor written; what holds it below the copy rate was not measured.\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
