#!/usr/bin/env python3
"""Times and quality of the map-plane fast mode (LOCGPU_P2PLANE_MAP) beside P2PLANE — both measured in the SAME
process on the SAME inputs; every ratio is against the existing method of this very build, never against an old record. Host clock
around synchronous calls for whole calls, the library's event timers (locgpu_profile_enable) for per-iteration stage times.

Steps (each a child process of its own with its own time limit; the run stops at the first step that fails):
  ingest_1m / ingest_10m   locgpu_icp_build_map_planes next to locgpu_icp_set_target (host tree build + H2D) of the same target;
  iteration                per-iteration search and accumulate times, one 115 200-point scan and a 256-scan batch, 10 M-point map;
                           plus the final distance to the true pose and the iteration count of both methods over the bench's
                           first 20 scans (quality);
  init_search              the 175-candidate initial-pose search of DESIGN §9 (4 000-point scan, 1 M-point local map).

    python3 tools/map_plane_time.py [--json profiles/map_planes.json] [--md profiles/map_planes.md] [--distinct 32]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("ingest_1m", 300), ("ingest_10m", 420), ("iteration", 600), ("init_search", 300)]


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4), reps=reps)


def pose_delta(a, b):
    dt = float(np.linalg.norm(a[4:] - b[4:]))
    d = abs(float(np.dot(a[:4] / np.linalg.norm(a[:4]), b[:4] / np.linalg.norm(b[:4]))))
    return dt, 2.0 * float(np.arccos(min(1.0, d)))


def step_ingest(api, synth, n_points, a):
    m = synth.make_local_map(n_points, 7, half=40) if n_points <= 1_000_000 else synth.make_map(n_points)
    ctx = api.Context(0)
    r = dict(points=len(m))
    t_set, t_build = [], []
    for _ in range(1 + a.reps_ingest):  # the first round allocates (reported apart)
        t0 = time.perf_counter(); ctx.icp_set_target(m); t1 = time.perf_counter(); ctx.icp_build_map_planes(); t2 = time.perf_counter()
        t_set.append(1e3 * (t1 - t0)); t_build.append(1e3 * (t2 - t1))
    r["set_target_ms_first"], r["build_map_planes_ms_first"] = round(t_set[0], 2), round(t_build[0], 2)
    r["set_target_ms_median"], r["build_map_planes_ms_median"] = round(float(np.median(t_set[1:])), 2), round(float(np.median(t_build[1:])), 2)
    r["build_over_set_target"] = round(r["build_map_planes_ms_median"] / r["set_target_ms_median"], 3)
    r.update({"planes_" + k: v for k, v in ctx.icp_map_planes_info().items()})
    ctx.close()
    return r


def stage_times(ctx, fn):
    ctx.profile_enable(1)
    ctx.profile_read(reset=True)
    fn()
    p = ctx.profile_read(reset=True)
    ctx.profile_enable(0)
    # locgpu_profile_read reports averages per launch
    return dict(search_ms_per_iter=round(p["search_ms"], 4), accum_ms_per_iter=round(p["accum_ms"], 4), solve_ms_per_iter=round(p["solve_ms"], 4),
                iterations_timed=p["search_n"])


def step_iteration(api, synth, a):
    ctx = api.Context(0)
    ctx.icp_set_target(synth.make_map(10_000_000))
    ctx.icp_build_map_planes()
    methods = dict(P2PLANE=api.icp_opts(method=api.P2PLANE), P2PLANE_MAP=api.icp_opts(method=api.P2PLANE_MAP))
    ids = list(range(max(a.distinct, 20)))
    scans = {i: synth.make_scan(i) for i in ids}
    poses = {i: synth.make_pose(i) for i in ids}
    r = dict(points_per_scan=len(scans[0]), distinct_scans=len(ids))
    one = {}
    for name, o in methods.items():
        ctx.icp_align(scans[0], poses[0][1], o)  # warm
        one[name] = stage_times(ctx, lambda: ctx.icp_align(scans[0], poses[0][1], o))
        one[name]["align_call"] = timed(lambda: ctx.icp_align(scans[0], poses[0][1], o), 1, a.reps)
    r["one_scan"] = one
    batch_ids = [ids[i % len(ids)] for i in range(a.batch)]
    b = ctx.batch([scans[i] for i in batch_ids])
    inits = np.stack([poses[i][1] for i in batch_ids])
    bt = {}
    for name, o in methods.items():
        ctx.icp_align_batch(b, inits, o)  # warm
        bt[name] = stage_times(ctx, lambda: ctx.icp_hb_batch(b, inits, o))  # ONE evaluation over all scans of the batch: a full-width iteration
        bt[name]["align_batch_call"] = timed(lambda: ctx.icp_align_batch(b, inits, o), 0, max(2, a.reps // 2))
    b.close()
    for part in (one, bt):
        for k in ("search_ms_per_iter", "accum_ms_per_iter"):
            part["ratio_" + k] = round(part["P2PLANE_MAP"][k] / part["P2PLANE"][k], 4) if part["P2PLANE"][k] else None
    r["batch"] = dict(scans=a.batch, **bt)
    q = {}
    for name, o in methods.items():
        rows = []
        for i in range(20):
            pose, st = ctx.icp_align(scans[i], poses[i][1], o)
            dt, dr = pose_delta(pose, poses[i][0])
            rows.append((dt, dr, st["iterations"], int(st["converged"])))
        rows = np.array(rows)
        q[name] = dict(dist_m_median=round(float(np.median(rows[:, 0])), 5), dist_m_max=round(float(rows[:, 0].max()), 5),
                       rot_rad_median=round(float(np.median(rows[:, 1])), 6), rot_rad_max=round(float(rows[:, 1].max()), 6),
                       iterations_mean=round(float(rows[:, 2].mean()), 2), iterations_max=int(rows[:, 2].max()), converged=int(rows[:, 3].sum()))
    d0 = np.array([pose_delta(poses[i][1], poses[i][0]) for i in range(20)])
    q["start"] = dict(dist_m_median=round(float(np.median(d0[:, 0])), 5), rot_rad_median=round(float(np.median(d0[:, 1])), 6))
    r["quality_20_scans"] = q
    ctx.close()
    return r


def step_init_search(api, synth, a):
    ctx = api.Context(0)
    ctx.icp_set_target(synth.make_local_map(1_000_000, 7, half=40))
    ctx.icp_build_map_planes()
    scan = synth.make_scan(7, crop_half=30, subsample=4000)
    true7, init7 = synth.make_pose(7)
    centre = init7.copy()
    centre[4:] += [1.3, -0.9, 0.0]
    cands, n = api.pose_grid(centre, 2.0, 1.0, 0.15, 0.05)
    r = dict(points=len(scan), candidates=int(n))
    for name, method in (("P2PLANE", api.P2PLANE), ("P2PLANE_MAP", api.P2PLANE_MAP)):
        o = api.icp_opts(method=method)
        t = timed(lambda: ctx.icp_init_search(scan, cands, o), a.warm, a.reps)
        poses, fit, stats, best = ctx.icp_init_search(scan, cands, o)
        t["best"] = best
        t["iterations_mean"] = round(float(np.mean([s["iterations"] for s in stats])), 2)
        if best >= 0:
            t["best_dist_to_true_m"], t["best_rot_to_true_rad"] = (round(v, 5) for v in pose_delta(poses[best], true7))
            t["best_score"] = fit[best]["score"]
        r[name] = t
    r["ratio_ms"] = round(r["P2PLANE_MAP"]["ms_median"] / r["P2PLANE"]["ms_median"], 4)
    ctx.close()
    return r


def write_md(res, path):
    L = ["# Map-plane fast mode (LOCGPU_P2PLANE_MAP) beside P2PLANE", "",
         "Same process, same inputs, this build; written by `tools/map_plane_time.py`. A labelled fast mode: none of this is a parity or headline figure.", ""]
    for k in ("ingest_1m", "ingest_10m"):
        if k in res:
            r = res[k]
            L.append("- **%s**: %d points; `icp_set_target` %.1f ms, `icp_build_map_planes` %.1f ms (first call %.1f ms), ratio %.3f; %d rows, %d valid, %.1f MB."
                     % (k, r["points"], r["set_target_ms_median"], r["build_map_planes_ms_median"], r["build_map_planes_ms_first"], r["build_over_set_target"],
                        r["planes_rows"], r["planes_valid"], r["planes_bytes"] / 1e6))
    if "iteration" in res:
        it = res["iteration"]
        for part, label in (("one_scan", "one %d-point scan" % it["points_per_scan"]), ("batch", "%d-scan batch (%d distinct scans)" % (it["batch"]["scans"], it["distinct_scans"]))):
            p = it[part]
            L.append("- **iteration, %s**: search %.3f -> %.3f ms (x%.3f), accumulate %.3f -> %.3f ms (x%.3f) per iteration, P2PLANE -> P2PLANE_MAP."
                     % (label, p["P2PLANE"]["search_ms_per_iter"], p["P2PLANE_MAP"]["search_ms_per_iter"], p["ratio_search_ms_per_iter"] or 0,
                        p["P2PLANE"]["accum_ms_per_iter"], p["P2PLANE_MAP"]["accum_ms_per_iter"], p["ratio_accum_ms_per_iter"] or 0))
        q = it["quality_20_scans"]
        for name in ("P2PLANE", "P2PLANE_MAP"):
            L.append("- **quality, %s, 20 scans**: distance to the true pose median %.4f m (max %.4f), rotation median %.5f rad; iterations mean %.2f (max %d), %d of 20 converged (start: %.3f m)."
                     % (name, q[name]["dist_m_median"], q[name]["dist_m_max"], q[name]["rot_rad_median"], q[name]["iterations_mean"], q[name]["iterations_max"], q[name]["converged"], q["start"]["dist_m_median"]))
    if "init_search" in res:
        s = res["init_search"]
        L.append("- **init search, %d candidates x %d points**: %.1f -> %.1f ms (x%.3f); mean iterations %.2f -> %.2f; winner %.4f m -> %.4f m from the true pose."
                 % (s["candidates"], s["points"], s["P2PLANE"]["ms_median"], s["P2PLANE_MAP"]["ms_median"], s["ratio_ms"], s["P2PLANE"]["iterations_mean"],
                    s["P2PLANE_MAP"]["iterations_mean"], s["P2PLANE"].get("best_dist_to_true_m", float("nan")), s["P2PLANE_MAP"].get("best_dist_to_true_m", float("nan"))))
    if res.get("failed"):
        L.append("- **stopped** at step `%s`: %s" % (res["failed"]["step"], res["failed"]["why"]))
    open(path, "w").write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "map_planes.json"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "map_planes.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-ingest", type=int, default=2)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32, help="distinct scans the 256-scan batch cycles through (bench.py uses 256)")
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS))
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        from loc_lib_amd import api, synth
        fn = dict(ingest_1m=lambda: step_ingest(api, synth, 1_000_000, a), ingest_10m=lambda: step_ingest(api, synth, 10_000_000, a),
                  iteration=lambda: step_iteration(api, synth, a), init_search=lambda: step_init_search(api, synth, a))[a.step]
        print("RESULT " + json.dumps(fn()), flush=True)
        return 0
    res = {}
    wanted = a.steps.split(",")
    for name, limit in STEPS:
        if name not in wanted:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--reps-ingest", str(a.reps_ingest), "--warm", str(a.warm),
               "--batch", str(a.batch), "--distinct", str(a.distinct)]
        print("step %s (limit %d s)" % (name, limit), flush=True)
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            res["failed"] = dict(step=name, why="time limit of %d s" % limit)
            break
        line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
        if out.returncode != 0 or not line:  # a fault, an abort or an error: nothing more is started on the GPU
            res["failed"] = dict(step=name, why="exit status %d: %s" % (out.returncode, (out.stderr or out.stdout)[-400:]))
            break
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(res, open(a.json, "w"), indent=1)
    write_md(res, a.md)
    return 1 if res.get("failed") else 0


if __name__ == "__main__":
    sys.exit(main())
