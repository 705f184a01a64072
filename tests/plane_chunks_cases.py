"""Inputs shared by tests/test_plane_chunks_ref.py (CPU) and tests/test_gpu_plane_chunks.py (GPU): scans whose LEADER COUNT PER
1 024-POINT BLOCK is designed, for the plane kernel that parks every leader's neighbour list in the plane table and fits the leaders
64 to a wave (plane_accum_flagged, csrc/icp_fit.hip).

A map is five-point clusters 8 m apart (plane patches of radius 0.3 m, 1 cm of noise, any orientation), as in
tests/icp_hb_cases.py: a query within 5 cm of a cluster's centre has exactly that cluster as its five nearest neighbours, under the
exact and under the approximate search. Every scan point sits near ONE chosen cluster, so the sequence of clusters sets the runs: a
point leads when it is lane 0 of its group of 64 or when its cluster is not the cluster of the point before it (tests/run_flags_ref.py).
A 1 024-point block therefore has at least 16 leaders.

Two maps. The search stage also flags every query it hands to its deep pass, and the point behind it, as leaders. Over WIDE_CLUSTERS
(300) clusters it hands over about 2 % of these queries (measured: 209 leaders more than designed per scan), so there the flagged
leaders are the designed ones and some more. The counts per block are exact only where no query goes that way: the map of N_CLUSTERS
(24) clusters, 120 points, a tree seven levels deep, as the 120-point map of tests/test_gpu_run_flags.py is. The designed counts are
asserted on that map, with the search stage's counters showing that no query left the walk kernel; the wide map has the same scan
with leaders of the other kind mixed in.

designed_scan(): seven blocks of 1 024 points with 16, 63, 64, 65, 128, 129 and 1 024 leaders — one chunk of 64 with three waves left
without one; the edges of the first and of the second chunk; every row of the table parked and overwritten.
"""
import numpy as np

N_CLUSTERS = 24
WIDE_CLUSTERS = 300
POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.05, -0.03, 0.02])
BLOCK_LEADERS = (16, 63, 64, 65, 128, 129, 1024)  # per 1 024-point block of the designed scan
# shared entries of the designed scan (28 blocks of 256 points, 112 walk waves) per points-per-thread rung of icp_accum_split: more than
# 2 048 walk waves in every case (the 64-lane walk kernel, which writes the flags); 532, 2 072 and 4 116 blocks of 256
RUNG_ENTRIES = {1: 19, 2: 74, 4: 147}
RAGGED_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
LONG = 4100          # the long scan of the ragged batches: 17 blocks of 256, 65 walk waves, five blocks of 1 024
RAGGED_SCANS = {1: 32, 4: 241}  # scans per ragged batch and rung: 32 × 65 = 2 080 waves, 544 blocks; 241 × 17 = 4 097 blocks
NOLIST = (1800, 90, 512)  # the four-point map: points (29 waves, 8 blocks), entries at 1 point per thread, entries at 4


def cluster_map(n=N_CLUSTERS, seed=31):
    """float32 [5 · n, 3]; cluster c holds rows 5c … 5c + 4."""
    rng = np.random.RandomState(seed)
    pts = []
    for c in range(n):
        ix, iy = c % 20, c // 20
        cen = np.array([(ix - 9.5) * 8.0 + rng.uniform(-0.5, 0.5), (iy - 7.0) * 8.0 + rng.uniform(-0.5, 0.5), rng.uniform(-3.0, 3.0)])
        f, _ = np.linalg.qr(rng.randn(3, 3))
        ang, rad = rng.uniform(0, 2 * np.pi, 5), 0.3 * np.sqrt(rng.uniform(0.05, 1.0, 5))
        pts.append(cen + np.outer(rad * np.cos(ang), f[:, 0]) + np.outer(rad * np.sin(ang), f[:, 1]) + np.outer(0.01 * rng.randn(5), f[:, 2]))
    return np.concatenate(pts).astype(np.float32)


def scan_of(m, clusters, seed):
    """One source point per entry of `clusters`, which POSE carries to within 5 cm of that cluster's centre. float32 [n, 3]."""
    rng = np.random.RandomState(seed)
    cen = m.astype(np.float64).reshape(-1, 5, 3).mean(axis=1)
    n = len(clusters)
    off = rng.randn(n, 3)
    off *= (0.05 * rng.uniform(0.2, 1.0, n) / np.linalg.norm(off, axis=1))[:, None]
    return (cen[np.asarray(clusters)] + off - POSE[4:]).astype(np.float32)


def sequence(block_leaders, seed, n_clusters=N_CLUSTERS):
    """(cluster [1024 · len], lead [1024 · len] bool): per 1 024-point block the given number of leaders — the 16 lane-0 points, which
    keep the cluster of the point before them, and points drawn from the others (lanes 1 and 63 of the block's first group among them
    when there is room), where the cluster changes."""
    rng = np.random.RandomState(seed)
    cluster, lead = [], []
    c = 0
    for n_lead in block_leaders:
        assert 16 <= n_lead <= 1024
        is_lead = (np.arange(1024) % 64) == 0
        free = np.flatnonzero(~is_lead)
        extra = n_lead - 16
        forced = [p for p in (1, 63) if extra >= 2]
        rest = np.setdiff1d(free, forced)
        chosen = np.concatenate([np.array(forced, dtype=int), rng.choice(rest, extra - len(forced), replace=False)]) if extra else np.array([], dtype=int)
        change = np.zeros(1024, dtype=bool)
        change[chosen] = True
        for k in range(1024):
            if change[k]:
                c = (c + 1) % n_clusters
            cluster.append(c)
        lead.append(is_lead | change)
    return np.array(cluster), np.concatenate(lead)


def designed_scan(m):
    """(scan [7 168, 3], lead [7 168] bool)."""
    cluster, lead = sequence(BLOCK_LEADERS, seed=5, n_clusters=len(m) // 5)
    return scan_of(m, cluster, seed=6), lead


def ragged_scans(m, n_scans):
    """(scans, lead per scan): the RAGGED_COUNTS cut from a sequence of mixed blocks at a multiple of 64 (a group of 64 of the cut is
    one of the sequence), an EMPTY scan, the LONG scan beside it, a scan with non-finite points between leaders, then copies of the
    long scan up to n_scans."""
    cluster, lead = sequence((129, 64, 1024, 65, 16), seed=8)
    pts = scan_of(m, cluster, seed=9)
    scans = [pts[192:192 + n] for n in RAGGED_COUNTS]
    leads = [lead[192:192 + n] for n in RAGGED_COUNTS]
    scans.append(pts[:0])
    leads.append(lead[:0])
    scans.append(pts[:LONG])
    leads.append(lead[:LONG])
    hostile = pts[1024 + 64:1024 + 64 + 200].copy()  # from the block of 64 leaders
    hostile[70] = (np.nan, 1.0, 2.0)
    hostile[71] = (np.inf, 0.0, 0.0)
    hostile[130] = (0.0, -np.inf, 1.0)
    scans.append(hostile)
    leads.append(None)  # a non-finite query is answered by the exact kernel: it and the point behind it lead, whatever their lists
    while len(scans) < n_scans:
        scans.append(pts[:LONG])
        leads.append(lead[:LONG])
    return scans, leads


def brute_nn(m, scan):
    """The five nearest map points of every scan point under POSE, exact, float64. int [n, 5]."""
    q, mm = scan.astype(np.float64) + POSE[4:], m.astype(np.float64)
    out = np.zeros((len(q), 5), dtype=np.int64)
    for a in range(0, len(q), 512):
        d = ((q[a:a + 512, None, :] - mm[None, :, :]) ** 2).sum(axis=2)
        out[a:a + 512] = np.argsort(d, axis=1, kind="stable")[:, :5]
    return out


def per_block(lead, block=1024):
    """Leaders per block of `block` points."""
    return [int(lead[i:i + block].sum()) for i in range(0, len(lead), block)]
