#!/usr/bin/env python3
"""Times of the fitness score and the initial-pose search (include/locgpu.h: locgpu_icp_fitness, locgpu_icp_init_search) beside the
nearest existing work. Host clock around the synchronous calls (each ends in a stream synchronisation), warm-up calls first, then
`--reps` repeats: median, min, max.

  fitness      one 115 200-point scan against the 10 M-point map, next to one P2P locgpu_icp_hb on the same inputs (one k = 1 search
               plus one reduction — but the alpha-pruned search of the defaults, where the score walks exactly);
  search_175   175 candidates of a 4 000-point scan against a 1 M-point local map, P2Plane, reference defaults;
  search_256   256 candidates of the 115 200-point scan against the 10 M-point map, next to locgpu_icp_align_batch on a batch of
               256 uploaded copies (+ the score on that batch), whose upload (472 MB) is reported separately.

--only-baseline runs just the parts that exist without the feature (icp_hb, the batch of copies): with LOCGPU_LIB set to a build
of the parent commit this gives its figures in the same session; --parent-lib PATH does that in a child process.

    python3 tools/init_search_time.py --out build/init_search_time.json [--parent-lib build_variants/parent/liblocgpu.so]
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


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "init_search_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only-baseline", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 10 M-point map workloads")
    a = ap.parse_args()
    from loc_lib_amd import api, synth
    res = dict(library=os.environ.get("LOCGPU_LIB") or "in-tree", only_baseline=a.only_baseline)
    ctx = api.Context(0)
    p2p, plane = api.icp_opts(method=api.P2P), api.icp_opts(method=api.P2PLANE)

    def grid(centre, xy_half, yaw_half):  # numpy restatement of locgpu_pose_grid (the parent build has none), 1 m / 0.05 rad steps
        kxy, kyaw = int(np.floor(xy_half + 1e-9)), int(np.floor(yaw_half / 0.05 + 1e-9))
        x, y, z, w = centre[:4]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z)], [2 * (x * z - y * w), 2 * (y * z + x * w)]])
        out = []
        for k in range(-kyaw, kyaw + 1):
            s, c = np.sin(0.025 * k), np.cos(0.025 * k)
            q = [x * c + y * s, -x * s + y * c, w * s + z * c, w * c - z * s]
            out += [np.concatenate([q, centre[4:] + R @ [float(i), float(j)]]) for i in range(-kxy, kxy + 1) for j in range(-kxy, kxy + 1)]
        return np.array(out)

    def search_case(name, scan, cands, opts):
        r = dict(points=len(scan), candidates=len(cands))
        if not a.only_baseline:
            r["init_search"] = timed(lambda: ctx.icp_init_search(scan, cands, opts), a.warm, a.reps)
        t0 = time.perf_counter()
        b = ctx.batch([scan] * len(cands))
        r["copies_upload_ms_once"] = round(1e3 * (time.perf_counter() - t0), 3)
        r["copies_upload_bytes"] = 16 * len(scan) * len(cands)
        r["copies_align_batch"] = timed(lambda: ctx.icp_align_batch(b, cands, opts), a.warm, a.reps)
        if not a.only_baseline:
            poses, _ = ctx.icp_align_batch(b, cands, opts)
            r["copies_fitness_batch"] = timed(lambda: ctx.icp_fitness_batch(b, poses, 1.0), a.warm, a.reps)
            sp, sf, _, _ = ctx.icp_init_search(scan, cands, opts, raw=True)
            r["bit_identical_to_copies"] = bool(sp.tobytes() == poses.tobytes() and bytes(sf) == bytes(ctx.icp_fitness_batch(b, poses, 1.0, raw=True)))
        b.close()
        res[name] = r
        print(name, json.dumps(r), flush=True)

    true7, init7 = synth.make_pose(7)
    centre = init7.copy()
    centre[4:] += [1.3, -0.9, 0.0]
    ctx.icp_set_target(synth.make_local_map(1_000_000, 7, half=40))
    search_case("search_175", synth.make_scan(7, crop_half=30, subsample=4000), grid(centre, 2.0, 0.15), plane)
    if not a.skip_large:
        ctx.icp_set_target(synth.make_map(10_000_000))
        s0 = synth.make_scan(0)
        _, init0 = synth.make_pose(0)
        r = dict(points=len(s0), icp_hb_p2p=timed(lambda: ctx.icp_hb(s0, init0, p2p), a.warm, a.reps))
        if not a.only_baseline:
            r["icp_fitness"] = timed(lambda: ctx.icp_fitness(s0, init0, 1.0), a.warm, a.reps)
            r["ratio_to_icp_hb"] = round(r["icp_fitness"]["ms_median"] / r["icp_hb_p2p"]["ms_median"], 3)
        res["fitness"] = r
        print("fitness", json.dumps(r), flush=True)
        search_case("search_256", s0, grid(init0, 2.0, 0.25)[:256], plane)
    ctx.close()
    if a.parent_lib and not a.only_baseline:
        env = dict(os.environ, LOCGPU_LIB=os.path.abspath(a.parent_lib))
        out = a.out + ".parent"
        cmd = [sys.executable, os.path.abspath(__file__), "--only-baseline", "--out", out, "--reps", str(a.reps), "--warm", str(a.warm)] + (["--skip-large"] if a.skip_large else [])
        subprocess.run(cmd, env=env, check=True, timeout=900)  # a fresh child process: its own library, its own GPU context
        res["parent_commit"] = json.load(open(out))
        os.remove(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
