"""Times the LOAM streaming loop (profiles/loam_stream.md): Lio::AddCloud(FullCloudPtr) per scan — upload, feature picker, voxel filter
of both classes, ScanMatch, and on keyframes the pair of local maps and SetInputTarget — once RESIDENT (locgpu_loam_scan_match_cloud,
locgpu_loam_submap_*, locgpu_loam_set_target_cloud) and once composed from the HOST-POINTER matcher entry points, which is what a
caller had before: the picker's clouds are downloaded and handed to locgpu_loam_scan_match with a host output cloud, the keyframe's
features are uploaded again for the maps, and both maps are downloaded for locgpu_loam_set_target. Same process, same library, the two
loops alternate; scans are the first 16 rings (28 800 points) of synth.make_scan(i), leaf 0.5, a keyframe on every second scan, two
keyframes in the maps. Per-scan time = wall time of scans 1..n-1 of one loop / (n - 1); warm-up loops excluded; median over the
repeated loops. Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from loc_lib_amd import api, synth  # noqa: E402

N_PTS, NUM_SCAN, LEAF, NUM_KFS = 28800, 16, 0.5, 2


def _inputs(n):
    out = []
    ring = (np.arange(N_PTS) // 1800).astype(np.uint8)
    for i in range(n):
        c = np.zeros((N_PTS, 4), np.float32)
        c[:, :3] = synth.make_scan(i)[:N_PTS, :3]
        truth, init = synth.make_pose(i)
        out.append((c, ring, np.array(truth, dtype=np.float64), np.array(init, dtype=np.float64)))
    return out


def loop(ctx, inputs, resident):
    """One pass over the scans; returns (seconds spent on scans 1.., poses, iterations)."""
    h = api.Loam()
    sub = api.LoamSubmap(ctx, NUM_KFS, LEAF)
    raw, out = api.Cloud(ctx), api.Cloud(ctx)
    poses, iters = [], []
    t0 = None
    try:
        for i, (c, ring, truth, init) in enumerate(inputs):
            if i == 1:
                t0 = time.perf_counter()
            raw.upload(c)
            edge, surf = raw.loam_extract(ring, NUM_SCAN)
            if i == 0:
                pose = truth
            else:
                edge.voxel_filter(LEAF, out=edge)
                surf.voxel_filter(LEAF, out=surf)
                if resident:
                    pose, st = h.scan_match_cloud(edge, surf, init, out=out)
                else:
                    e, s = edge.download(), surf.download()
                    pose, st, _ = h.scan_match(e, s, init, out_cloud=np.empty((len(e) + len(s), 4), np.float32))
                poses.append(pose)
                iters.append(st["iterations"])
            if i % 2 == 0:
                if resident:
                    sub.add_keyframe(edge, surf, pose)
                    h.set_target_cloud(*sub.clouds())
                else:
                    if i > 0:  # the features left the device for the match: the keyframe is made of a second upload
                        edge, surf = api.Cloud(ctx, e), api.Cloud(ctx, s)
                    sub.add_keyframe(edge, surf, pose)
                    em, sm = sub.clouds()
                    h.set_target(em.download(), sm.download())
        api.lib().locgpu_loam_last_error(h._h)  # every call above is synchronous: nothing is left in flight
        return time.perf_counter() - t0, np.array(poses), iters
    finally:
        sub.close()
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=13)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    inputs = _inputs(a.scans)
    ctx = api.Context(0)
    ms = {True: [], False: []}
    ref = {}
    for r in range(-a.warmup, a.reps):
        for resident in (True, False):
            sec, poses, iters = loop(ctx, inputs, resident)
            ref.setdefault(resident, (poses, iters))
            assert np.array_equal(poses, ref[resident][0])  # a loop repeats itself bit for bit
            if r >= 0:
                ms[resident].append(1e3 * sec / (a.scans - 1))
    assert np.array_equal(ref[True][0], ref[False][0]) and ref[True][1] == ref[False][1]  # and the two loops compute the same poses
    ctx.close()

    def q(v):
        v = np.sort(np.asarray(v))
        return dict(n=len(v), min_ms=float(v[0]), median_ms=float(v[len(v) // 2]), max_ms=float(v[-1]))
    print(json.dumps(dict(scans=a.scans, points_per_scan=N_PTS, warmup_loops=a.warmup, iterations=ref[True][1],
                          resident_per_scan=q(ms[True]), host_pointer_per_scan=q(ms[False]))))


if __name__ == "__main__":
    main()
