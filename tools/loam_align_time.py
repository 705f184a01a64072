"""Times the LOAM matcher (profiles/loam_align.md): LoamRegistration::ScanMatch through the façade — tools/ubench/loam_facade_time, one
or several builds of it given as --exe LABEL=PATH — and locgpu_loam_align_batch on 64 scans against 64 sequential locgpu_loam_scan_match
calls. Two inputs: the small world's edge / surface split of the tests, and the clouds the GPU feature picker extracts from 115 200-point
scans, against maps extracted the same way (the features of six consecutive scans of the circuit, the matched ones among them, moved into the
world frame by their true poses).
Prints one JSON object; every timing is host wall time around synchronous calls, warm-up excluded, with min / p10 / median / p90."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from loc_lib_amd import api, synth  # noqa: E402


def _quantiles(ms):
    ms = np.sort(np.asarray(ms))
    return dict(n=len(ms), min_ms=float(ms[0]), p10_ms=float(ms[int(0.1 * len(ms))]), median_ms=float(ms[len(ms) // 2]), p90_ms=float(ms[min(len(ms) - 1, int(0.9 * len(ms)))]))


def _features(ctx, scan_id):
    s = synth.make_scan(scan_id)
    c = np.zeros((len(s), 4), np.float32)
    c[:, :3] = s[:, :3]
    ring = (np.arange(len(s)) // 1800).astype(np.uint8)
    edge, surf = api.Cloud(ctx, c).loam_extract(ring, 64)
    return np.ascontiguousarray(edge.download()[:, :3]), np.ascontiguousarray(surf.download()[:, :3]), len(s)


def small_world_input():
    m = synth.make_local_map(200000, 3, half=40.0)
    s = synth.make_scan(3, subsample=10000, crop_half=36.0)
    _, init = synth.make_pose(3)
    return dict(edge_map=m[::5], surf_map=m, scans=[(s[::7], s[np.arange(len(s)) % 7 != 0], np.array(init))])


def picker_input(ctx, scan_ids, map_ids, poses_per_scan, seed=11):
    em, sm = [], []
    for i in map_ids:
        e, s, _ = _features(ctx, i)
        true_pose, _ = synth.make_pose(i)
        em.append(ctx.transform_cloud(true_pose, e))
        sm.append(ctx.transform_cloud(true_pose, s))
    rng = np.random.RandomState(seed)
    scans, n_points = [], 0
    for i in scan_ids:
        e, s, n_points = _features(ctx, i)
        _, init = synth.make_pose(i)
        scans.append((e, s, np.array(init)))
        for _ in range(poses_per_scan - 1):  # the same feature clouds from further predictions around the first
            dx = np.concatenate([rng.uniform(-0.005, 0.005, 3), rng.uniform(-0.1, 0.1, 3)])
            scans.append((e, s, api.gn_update(np.concatenate([np.eye(6).reshape(-1), dx, [1e18, 1.0]]), api.P2PLANE, 0, 0.0, np.array(init))[0]))
    return dict(edge_map=np.vstack(em), surf_map=np.vstack(sm), scans=scans, points_per_scan=n_points)


def time_facade(exes, inp, warmup, reps):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        e, s, init = inp["scans"][0]
        for name, arr in (("em", inp["edge_map"]), ("sm", inp["surf_map"]), ("e", e), ("s", s)):
            np.ascontiguousarray(arr[:, :3], dtype=np.float32).tofile(os.path.join(d, name + ".bin"))
        np.asarray(init, dtype=np.float64).tofile(os.path.join(d, "pose.bin"))
        for label, exe in exes:
            r = subprocess.run([exe] + [os.path.join(d, n + ".bin") for n in ("em", "sm", "e", "s", "pose")] + [str(warmup), str(reps)], capture_output=True, text=True, timeout=900)
            out[label] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode in (0, 3) and r.stdout.strip() else dict(error=r.returncode, stderr=r.stderr[-400:])
    return out


def time_abi(inp, warmup, reps):
    h = api.Loam()
    try:
        h.set_target(inp["edge_map"], inp["surf_map"])
        edges = [np.ascontiguousarray(x[0][:, :3], np.float32) for x in inp["scans"]]
        surfs = [np.ascontiguousarray(x[1][:, :3], np.float32) for x in inp["scans"]]
        inits = np.array([x[2] for x in inp["scans"]])
        res = dict(n_scans=len(edges), edge_points=[len(e) for e in edges][:4], surf_points=[len(s) for s in surfs][:4])
        one, seq, bat = [], [], []
        st0 = None
        for r in range(-warmup, reps):
            t0 = time.perf_counter()
            _, st0, _ = h.scan_match(edges[0], surfs[0], inits[0])
            if r >= 0:
                one.append(1e3 * (time.perf_counter() - t0))
        res["scan_match_one"] = dict(_quantiles(one), iterations=st0["iterations"], status=st0["status"], converged=st0["converged"])
        if len(edges) > 1:
            seq_stats = bat_stats = None
            for r in range(-max(1, warmup // 4), max(3, reps // 8)):
                t0 = time.perf_counter()
                seq_stats = [h.scan_match(e, s, p, out_cloud=np.zeros((0, 3), np.float32))[1] for e, s, p in zip(edges, surfs, inits)]
                t1 = time.perf_counter()
                _, bat_stats = h.align_batch(edges, surfs, inits)
                t2 = time.perf_counter()
                if r >= 0:
                    seq.append(1e3 * (t1 - t0))
                    bat.append(1e3 * (t2 - t1))
            res["sequential_scan_match"] = dict(_quantiles(seq), iterations=[s["iterations"] for s in seq_stats], status=[s["status"] for s in seq_stats])
            res["align_batch"] = dict(_quantiles(bat), iterations=[s["iterations"] for s in bat_stats], status=[s["status"] for s in bat_stats])
        return res
    finally:
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", action="append", default=[], help="LABEL=PATH of a loam_facade_time build; may be repeated")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    exes = [x.split("=", 1) for x in a.exe] or [["this", os.path.join(ROOT, "tools", "ubench", "loam_facade_time")]]
    ctx = api.Context(0)
    small = small_world_input()
    picker = picker_input(ctx, scan_ids=[2, 3, 4, 5], map_ids=[1, 2, 3, 4, 5, 6], poses_per_scan=max(1, a.batch // 4))
    ctx.close()
    out = dict(small_world=dict(facade=time_facade(exes, small, a.warmup, a.reps), abi=time_abi(small, a.warmup, a.reps)),
               picker=dict(points_per_scan=picker["points_per_scan"], map_points=[len(picker["edge_map"]), len(picker["surf_map"])],
                           facade=time_facade(exes, picker, a.warmup, a.reps), abi=time_abi(picker, a.warmup, a.reps)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
