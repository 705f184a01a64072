"""The plane kernel that parks every leader's neighbour list in its row of the plane table and fits the leaders 64 to a wave from
there (plane_accum_flagged, csrc/icp_fit.hip: the default) against the kernel that finds the runs itself and loads a leader's list in
its fit pass (LOCGPU_PLANE_RUNFLAGS=0) and, for the designed scan, against a fit per point (LOCGPU_PLANE_DEDUP=0): per scan H, B and
effective number of the ICP H/B evaluation call must be the same bits. The switches are read once per process, so each setting runs
tests/gpu_plane_chunks_case.py in a child process, once for the module, on the same inputs.

The inputs (tests/plane_chunks_cases.py) set the LEADER COUNT of every 1 024-point block — the smallest shapes at which parked lists
and 64-leader chunks can go wrong:
    (Every count below is exact on the 24-cluster map, where no query leaves the walk kernel; the designed scan runs over 300
    clusters as well, where the search stage's deep pass adds leaders of its own: see tests/plane_chunks_cases.py.)
    the designed scan   blocks of 16, 63, 64, 65, 128, 129 and 1 024 leaders: one chunk with three waves left without one, the edges of
                        the first two chunks, every table row parked and then overwritten by its plane. At 1, 2 and 4 points per
                        thread (19, 74 and 147 shared entries), where a block is 256, 512 and 1 024 of these points.
    ragged batches      counts 1, 63, 64, 65, 255, 256, 257, 1 023, 1 024, 1 025, an EMPTY scan beside a scan of 4 100 points (every
                        block of the empty scan lies past its count: no leader, no fit pass), a scan with NaN and inf points between
                        leaders; at 1 and at 4 points per thread, in one launch each.
    the four-point map  every point leads, none has a list: "no fit" for all of them with no look at the tree.
    ten repeats         of the designed batch in one process: all equal.
For every designed scan the leader count the design aims at is confirmed on the CPU (the numpy restatement, also
tests/test_plane_chunks_ref.py) and on the GPU (the flags read back through locgpu_debug_batch_run_flags).

A leader WITHOUT a full list between leaders that have one cannot be made through the API under P2Plane: the search fills all five
slots of every query — a non-finite one included — or, against a map of fewer than five points, none for the whole map (see
tests/test_gpu_plane_dedup.py). What can be made is here: the four-point map, and non-finite points, which the search stage flags
as leaders whatever their lists, between leaders with ordinary ones. That a parked list with an empty fifth slot gets the verdict
"no fit" and leaves its row alone is the same test on the same word as before (slot[4]), now read from the row."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_chunks_cases as pc
from run_flags_ref import leaders, unpack_flags

pytestmark = pytest.mark.gpu

N_NAMED = len(pc.RAGGED_COUNTS) + 3  # the counts, the empty scan, the long scan, the scan with non-finite points


@pytest.fixture(scope="module")
def inputs():
    m = pc.cluster_map()
    scan, lead = pc.designed_scan(m)
    d = dict(map=m, scan=scan, lead=lead, wide_map=pc.cluster_map(pc.WIDE_CLUSTERS))
    d["wide_scan"], _ = pc.designed_scan(d["wide_map"])
    for rung, n in pc.RAGGED_SCANS.items():
        d["ragged%d" % rung], d["ragged_lead%d" % rung] = pc.ragged_scans(m, n)
    return d


@pytest.fixture(scope="module")
def results(tmp_path_factory, inputs):
    """{setting: the child's .npz} for "default", "runflags0" and "dedup0" (the designed scan at four points per thread alone)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("plane_chunks")
    fin = str(tmp / "in.npz")
    blob = dict(map=inputs["map"], scan=inputs["scan"], wide_map=inputs["wide_map"], wide_scan=inputs["wide_scan"], pose=pc.POSE, rung_entries=np.array(sorted(pc.RUNG_ENTRIES.items())), nolist=np.array(pc.NOLIST))
    for rung in pc.RAGGED_SCANS:
        blob["n_ragged%d" % rung] = len(inputs["ragged%d" % rung])
        blob.update({"ragged%d_%d" % (rung, i): s for i, s in enumerate(inputs["ragged%d" % rung])})
    np.savez(fin, **blob)
    out = {}
    for setting, env, what in (("default", {}, "all"), ("runflags0", {"LOCGPU_PLANE_RUNFLAGS": "0"}, "all"), ("dedup0", {"LOCGPU_PLANE_DEDUP": "0"}, "designed")):
        fout = str(tmp / ("out_%s.npz" % setting))
        clean = {k: v for k, v in os.environ.items() if k not in ("LOCGPU_PLANE_RUNFLAGS", "LOCGPU_PLANE_DEDUP")}
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_plane_chunks_case.py"), fin, fout, what],
                           env=dict(clean, **env), capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[setting] = dict(np.load(fout))
    return out


def _same(results, key, other="runflags0"):
    on, off = results["default"][key], results[other][key]
    assert on.shape == off.shape
    return on, off


def test_the_design_on_the_cpu(inputs):
    """The restatement on exact neighbours marks the designed leaders: 16 … 1 024 per block of 1 024."""
    got = leaders(pc.brute_nn(inputs["map"], inputs["scan"]))
    assert np.array_equal(got, inputs["lead"]) and pc.per_block(got) == list(pc.BLOCK_LEADERS)
    for s, lead in list(zip(inputs["ragged1"], inputs["ragged_lead1"]))[:N_NAMED - 1]:
        if len(s):
            assert np.array_equal(leaders(pc.brute_nn(inputs["map"], s)), lead)


def test_the_flags_on_the_gpu_are_the_designed_leaders(results, inputs):
    res = results["default"]
    n = len(inputs["scan"])
    for rung, entries in pc.RUNG_ENTRIES.items():
        key = "x%d" % rung
        assert res["written_" + key] and not results["runflags0"]["written_" + key]
        flags = res["flags_" + key]
        assert flags.shape[0] == entries
        for e in range(entries):
            assert np.array_equal(unpack_flags(flags[e], n), inputs["lead"]), (key, e)
    print("designed scan: leaders per block of 1 024: %s" % pc.per_block(unpack_flags(res["flags_x4"][0], n)))
    assert pc.per_block(unpack_flags(res["flags_x4"][0], n)) == list(pc.BLOCK_LEADERS)
    searched, redone, walked = res["stats"]
    print("%d queries, %d answered exactly, %d through the deep pass" % (searched, redone, walked))
    assert redone == 0 and walked == 0  # the input is what it claims: every leader is a designed one
    _, redone, walked = res["stats_ragged"]
    assert walked == 0 and redone == 3 * len(pc.RAGGED_SCANS)  # … but for the three non-finite points of either ragged batch
    for rung in pc.RAGGED_SCANS:
        assert res["written_ragged%d" % rung]
        flags = res["flags_ragged%d" % rung]
        for i, (s, lead) in enumerate(zip(inputs["ragged%d" % rung], inputs["ragged_lead%d" % rung])):
            if lead is not None:
                assert np.array_equal(unpack_flags(flags[i], len(s)), lead), (rung, i)
        # the scan with non-finite points: they lead, the points behind them lead, and no designed leader is lost
        hostile = unpack_flags(flags[N_NAMED - 1], 200)
        assert hostile[[70, 71, 72, 130, 131]].all()
        want = leaders(pc.brute_nn(inputs["map"], np.nan_to_num(inputs["ragged%d" % rung][N_NAMED - 1], nan=0.0, posinf=0.0, neginf=0.0)))
        want[[70, 71, 72, 130, 131]] = True
        assert np.array_equal(hostile, want)


def test_hb_of_the_designed_scan_at_every_rung(results, inputs):
    n = len(inputs["scan"])
    for rung, entries in pc.RUNG_ENTRIES.items():
        on, off = _same(results, "hb_x%d" % rung)
        assert on.shape == (entries, 44) and np.isfinite(on).all()
        assert np.array_equal(on, off), rung
        assert (on == on[0]).all() and on[0, 43] == 1.0 and on[0, 42] == n  # every point has a fitted plane
    on, per_point = _same(results, "hb_x4", "dedup0")
    assert np.array_equal(on, per_point)


def test_the_designed_scan_over_three_hundred_clusters(results, inputs):
    """The same runs, with the leaders the search stage's deep pass makes among them: no designed leader is lost, the extra ones are
    at most two per deep or exact query, and the sums are the other kernel's bits."""
    res, n = results["default"], len(inputs["wide_scan"])
    assert res["written_wide"]
    searched, redone, walked = res["stats_wide"]
    flagged = 0
    for e in range(pc.RUNG_ENTRIES[4]):
        lead = unpack_flags(res["flags_wide"][e], n)
        assert not (inputs["lead"] & ~lead).any()
        flagged += int(lead.sum())
    designed = pc.RUNG_ENTRIES[4] * int(inputs["lead"].sum())
    print("300 clusters: %d flagged leaders, %d designed, %d deep or exact queries of %d" % (flagged, designed, redone + walked, searched))
    assert flagged - designed <= 2 * (redone + walked)
    on, off = _same(results, "hb_wide")
    assert np.array_equal(on, off) and np.isfinite(on).all() and (on == on[0]).all() and on[0, 42] == n


def test_hb_of_the_ragged_batches(results, inputs):
    k = len(pc.RAGGED_COUNTS)
    for rung, n_scans in pc.RAGGED_SCANS.items():
        on, off = _same(results, "hb_ragged%d" % rung)
        assert on.shape == (n_scans, 44)
        assert np.array_equal(on, off, equal_nan=True) and on.tobytes() == off.tobytes()
        assert on[:k, 42].tolist() == [float(c) for c in pc.RAGGED_COUNTS]  # every point of every cut has a fitted plane
        assert not on[k].any()  # the empty scan: exactly nothing
        assert on[k + 1, 42] == pc.LONG and np.isfinite(on[:k + 2]).all()
        assert 197.0 <= on[k + 2, 42] <= 200.0  # the three non-finite points keep whatever list the exact search gave them
        assert (on[k + 3:] == on[k + 1]).all()
        print("ragged, %d point(s) per thread: effective_num %s" % (rung, on[:k + 3, 42].astype(int).tolist()))


def test_a_map_of_four_points(results):
    """No query has a list. Every point is flagged a leader — 1 800 parked lists of five empty slots — and none fits: nothing is
    counted or summed, at 1 and at 4 points per thread."""
    points, e1, e4 = pc.NOLIST
    for key, n in (("nolist1", e1), ("nolist4", e4)):
        on, off = _same(results, "hb_" + key)
        assert on.shape == (n, 44) and np.array_equal(on, off) and not on.any()
        assert results["default"]["written_" + key]
        flags = results["default"]["flags_" + key]
        assert all(unpack_flags(flags[e], points).all() for e in range(n))
    assert (results["default"]["nn_nolist1"][:, :points, 4] == -1).all()  # four neighbours at the most: no full list


def test_ten_repeats_are_one_result(results):
    """The same H/B evaluation ten times in one process: which wave fitted which leader, and when, never shows."""
    runs = results["default"]["hb_repeats_x4"]
    assert runs.shape == (10, pc.RUNG_ENTRIES[4], 44)
    for r in range(1, 10):
        assert np.array_equal(runs[r], runs[0]), r
