"""tests/plane_chunks_cases.py — the designed inputs of tests/test_gpu_plane_chunks.py — do what they are for (no GPU): with the exact
five nearest neighbours worked out in numpy, the restatement of the run flags (tests/run_flags_ref.py) marks exactly the designed
leaders, and every 1 024-point block has the leader count the design aims at."""
import numpy as np

import plane_chunks_cases as pc
from run_flags_ref import leaders


def test_every_query_gets_its_own_cluster():
    for n in (pc.N_CLUSTERS, pc.WIDE_CLUSTERS):
        m = pc.cluster_map(n)
        cluster, _ = pc.sequence(pc.BLOCK_LEADERS, seed=5, n_clusters=n)
        nn = pc.brute_nn(m, pc.scan_of(m, cluster, seed=6))
        assert np.array_equal(np.sort(nn, axis=1), 5 * cluster[:, None] + np.arange(5))
        cen = m.astype(np.float64).reshape(-1, 5, 3).mean(axis=1)
        d = np.linalg.norm(cen[:, None] - cen[None], axis=2) + 1e9 * np.eye(len(cen))
        assert d.min() > 6.0  # clusters stay apart: the approximate search (alpha 0.1) has no second candidate


def test_leaders_per_block_of_the_designed_scan():
    wide, wide_lead = pc.designed_scan(pc.cluster_map(pc.WIDE_CLUSTERS))
    assert np.array_equal(leaders(pc.brute_nn(pc.cluster_map(pc.WIDE_CLUSTERS), wide)), wide_lead)
    m = pc.cluster_map()
    scan, lead = pc.designed_scan(m)
    assert np.array_equal(lead, wide_lead)  # the same runs over either map
    assert len(scan) == 1024 * len(pc.BLOCK_LEADERS) and -(-len(scan) // 256) == 28
    got = leaders(pc.brute_nn(m, scan))
    assert np.array_equal(got, lead)
    assert pc.per_block(got) == list(pc.BLOCK_LEADERS)
    # chunks of 64 leaders a block's four waves share: 1, 1, 1, 2, 2, 3 and 16
    assert [-(-n // 64) for n in pc.per_block(got)] == [1, 1, 1, 2, 2, 3, 16]
    # lanes 1 and 63 of a block's first group lead wherever the design had room for them
    for b, n in enumerate(pc.BLOCK_LEADERS):
        assert bool(lead[1024 * b + 1]) == bool(lead[1024 * b + 63]) == (n >= 18)


def test_rungs_and_walk_waves_of_the_batches():
    """icp_accum_split: fewer than 2 048 blocks of 256 points → 1 point per thread, fewer than 4 096 → 2, else 4; the 64-lane walk
    kernel (the one that writes flags) takes batches of more than 2 048 waves."""
    def rung(blocks):
        return 4 if blocks >= 4096 else 2 if blocks >= 2048 else 1
    for want, entries in pc.RUNG_ENTRIES.items():
        assert rung(28 * entries) == want and 112 * entries > 2048
    for want, n in pc.RAGGED_SCANS.items():
        assert rung(-(-pc.LONG // 256) * n) == want and -(-pc.LONG // 64) * n > 2048
    points, e1, e4 = pc.NOLIST
    assert rung(-(-points // 256) * e1) == 1 and rung(-(-points // 256) * e4) == 4 and -(-points // 64) * e1 > 2048


def test_leaders_of_the_ragged_scans():
    m = pc.cluster_map()
    scans, leads = pc.ragged_scans(m, pc.RAGGED_SCANS[1])
    assert [len(s) for s in scans[:len(pc.RAGGED_COUNTS) + 2]] == list(pc.RAGGED_COUNTS) + [0, pc.LONG]
    for s, lead in zip(scans[:len(pc.RAGGED_COUNTS) + 2], leads):
        if len(s):
            assert np.array_equal(leaders(pc.brute_nn(m, s)), lead)
    # the long scan: blocks of 129, 64, 1 024 and 65 leaders and four points of a fifth; the empty scan beside it leaves every block
    # of its own past the count
    assert pc.per_block(leads[len(pc.RAGGED_COUNTS) + 1]) == [129, 64, 1024, 65, 1]
    # the cuts start at point 192 of the first block: a count of 1 is one leader, 1 025 ends one point into the block of 64
    assert [int(l.sum()) for l in leads[:len(pc.RAGGED_COUNTS)]] == [int(leads[len(pc.RAGGED_COUNTS) + 1][192:192 + n].sum()) for n in pc.RAGGED_COUNTS]
    assert int(leads[0].sum()) == 1
