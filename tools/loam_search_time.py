#!/usr/bin/env python3
"""Wall time of one LOAM initial-pose search (include/locgpu.h: locgpu_loam_init_search) beside what the library offered for the same
job before it: locgpu_loam_align_batch on one host copy of the pair of scans per candidate, then 2 locgpu_icp_fitness calls per
candidate (surface and edge) on two plain contexts holding the same maps. Inputs: the small world's edge / surface split
(tests/loam_ref.py: 1 429 edge and 8 571 surface points against 40 000 / 200 000 map points) and 175 candidates (±2 m in 1 m steps,
±0.15 rad in 0.05 rad steps round the initial pose). Host clock round the synchronous calls (each ends in a stream synchronisation),
warm-up calls first, then `--reps` repeats: median, min, max. The baseline uses only calls the parent commit has, so LOCGPU_LIB set to
a build of it (with --only-baseline) gives its figures in the same session.

    python3 tools/loam_search_time.py --out build/loam_search_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "loam_search_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--eps", type=float, default=1e-3, help="LoamOption::eps_ (1e-3: the small world's loop runs to its 20-iteration cap)")
    ap.add_argument("--only-baseline", action="store_true")
    a = ap.parse_args()
    import loam_ref
    from loc_lib_amd import api, synth
    true_pose, init = synth.make_pose(3)
    w = loam_ref.split_world(dict(map=synth.make_local_map(200000, 3, half=40.0), scan10k=synth.make_scan(3, subsample=10000, crop_half=36.0), init_pose=init))
    cands, m = api.pose_grid(w["init"], 2.0, 1.0, 0.15, 0.05)
    assert m == 175
    res = dict(library=os.environ.get("LOCGPU_LIB") or "in-tree", candidates=m, edge_points=len(w["edge"]), surf_points=len(w["surf"]), eps=a.eps)
    h = api.Loam(api.loam_opts(eps=a.eps))
    h.set_target(w["edge_map"], w["surf_map"])
    surf_ctx, edge_ctx = api.Context(0), api.Context(0)
    surf_ctx.icp_set_target(w["surf_map"])
    edge_ctx.icp_set_target(w["edge_map"])
    edges, surfs = [w["edge"]] * m, [w["surf"]] * m

    def baseline():
        poses, stats = h.align_batch(edges, surfs, cands)
        fit = []
        for p in poses:  # what a caller of the parent commit writes: two scoring calls per candidate
            fit.append((surf_ctx.icp_fitness(w["surf"], p, 1.0, raw=True), edge_ctx.icp_fitness(w["edge"], p, 1.0, raw=True)))
        return poses, stats, fit

    res["baseline_align_batch_plus_350_icp_fitness"] = timed(baseline, a.warm, a.reps)
    res["baseline_align_batch_alone"] = timed(lambda: h.align_batch(edges, surfs, cands), a.warm, a.reps)
    if not a.only_baseline:
        res["loam_init_search"] = timed(lambda: h.init_search(w["edge"], w["surf"], cands), a.warm, a.reps)
        poses, stats, fit = baseline()
        sp, sf, ss, best = h.init_search(w["edge"], w["surf"], cands, raw=True)
        f = np.frombuffer(bytes(sf), dtype=[("score", "f8"), ("inliers", "i8"), ("finite_points", "i8")]).reshape(m, 3)
        same = sp.tobytes() == poses.tobytes() and ss == stats
        same = same and all(bytes(fit[i][0]) == f[i, 1].tobytes() and bytes(fit[i][1]) == f[i, 2].tobytes() for i in range(m))
        res["bit_identical_to_baseline"] = bool(same)
        res["best"] = best
        res["ratio_baseline_to_search"] = round(res["baseline_align_batch_plus_350_icp_fitness"]["ms_median"] / res["loam_init_search"]["ms_median"], 3)
    h.close()
    surf_ctx.close()
    edge_ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
