#!/usr/bin/env python3
"""How many plane fits of a scan are repeats (CPU only, the oracle's tree): for scans of the headline workload at their initial and
their true pose, the share of points whose five neighbours (`KdTree.knn(k=5, approximate=True, alpha=0.1)`, what the P2Plane search
finds) are the SET, or the ordered LIST, of the point before them; the distinct sets per 1024-point block; the leaders under the fit
kernel's rule (sorted list differs from the predecessor's, or lane 0 of a wave); the wave-passes a 1024-point block then needs when the
fits are dealt 64 to a wave; and the longest run. The figures of profiles/plane_dedup.md:

    python3 tools/plane_dedup_share.py [--map-points 10000000] [--scans 0 37 100 200]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def transform(pose, xyz):
    """pose = quaternion xyzw + t, applied in float64 and rounded to the float32 query the search kernel makes."""
    x, y, z, w = pose[:4] / np.linalg.norm(pose[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return (xyz.astype(np.float64) @ R.T + pose[4:]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=10_000_000)
    ap.add_argument("--scans", type=int, nargs="+", default=[0, 37, 100, 200])
    a = ap.parse_args()
    from loc_lib_amd import synth
    from oracle import locref

    tree = locref.KdTree(synth.make_map(a.map_points))
    print("scan pose    same set  same list  distinct sets / 1024  leaders  wave-passes / 16 (min..max)  longest run")
    for sid in a.scans:
        scan = synth.make_scan(sid)
        true_pose, init_pose = synth.make_pose(sid)
        for name, pose in (("init", init_pose), ("true", true_pose)):
            nn = tree.knn(transform(np.asarray(pose, dtype=np.float64), scan[:, :3]), k=5, approximate=True, alpha=0.1)
            srt = np.sort(nn, axis=1)
            same_set = np.r_[False, (srt[1:] == srt[:-1]).all(axis=1)]
            same_list = np.r_[False, (nn[1:] == nn[:-1]).all(axis=1)]
            leader = ~same_set | (np.arange(len(nn)) % 64 == 0)
            n_blocks = -(-len(nn) // 1024)
            distinct = np.mean([len(np.unique(srt[b * 1024:(b + 1) * 1024], axis=0)) / len(srt[b * 1024:(b + 1) * 1024]) for b in range(n_blocks)])
            passes = np.array([-(-int(leader[b * 1024:(b + 1) * 1024].sum()) // 64) for b in range(n_blocks - 1)])
            run, longest = 0, 0
            for s in same_set:
                run = run + 1 if s else 1
                longest = max(longest, run)
            print("%4d %-5s   %.3f     %.3f      %.3f                 %.3f    %.3f (%d..%d)               %d"
                  % (sid, name, same_set.mean(), same_list.mean(), distinct, leader.mean(), passes.mean() / 16.0, passes.min(), passes.max(), longest))


if __name__ == "__main__":
    main()
