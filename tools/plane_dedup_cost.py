#!/usr/bin/env python3
"""What LOCGPU_PLANE_DEDUP costs where it cannot win (run ON the GPU box): the fit / accumulate stage of the headline step — 256 scans
against the 10 M-point map, P2Plane, one alignment at a time with HIP events around every stage — with the scans as the sensor stores
them (ring-major: about half the points share their neighbour set with the point before them) and with every scan's points permuted by
a fixed seed (no two consecutive points share a set: every point is a leader and the dedup kernel's sort, rank and table are pure
overhead). The switch is read once per process, so dedup on and off are two calls:

    LOCGPU_PLANE_DEDUP=1 python3 tools/plane_dedup_cost.py [--scans 256] [--steps 4]
    LOCGPU_PLANE_DEDUP=0 python3 tools/plane_dedup_cost.py
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--map-points", type=int, default=10_000_000)
    a = ap.parse_args()
    from loc_lib_amd import api, synth

    ctx = api.Context(0)
    ctx.icp_set_target(synth.make_map(a.map_points))
    ids = [i % 256 for i in range(a.scans)]
    scans = [synth.make_scan(i) for i in ids]
    inits = np.stack([synth.make_pose(i)[1] for i in ids])
    opts = api.icp_opts(method=api.P2PLANE)
    rng = np.random.RandomState(20260)
    cases = (("ring order", scans), ("permuted", [np.ascontiguousarray(s[rng.permutation(len(s))]) for s in scans]))
    for name, sc in cases:
        b = ctx.batch(sc)
        try:
            poses, st = ctx.icp_align_batch(b, inits, opts)  # warm-up
            ctx.profile_read(reset=True)
            ctx.profile_enable(1)
            for _ in range(a.steps):
                ctx.icp_align_batch(b, inits, opts)
            p = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
        finally:
            b.close()
        print("LOCGPU_PLANE_DEDUP=%s  %-10s  fit/accumulate %.3f ms per step (%d launches per step), search %.3f ms, iterations %d"
              % (os.environ.get("LOCGPU_PLANE_DEDUP", "(default 1)"), name, p["accum_ms"] * p["accum_n"] / a.steps, p["accum_n"] // a.steps,
                 p["search_ms"] * p["search_n"] / a.steps, sum(s["iterations"] for s in st)))
    ctx.close()


if __name__ == "__main__":
    main()
