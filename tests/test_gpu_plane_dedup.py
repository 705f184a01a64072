"""icp_plane_accum_kernel<FIT, true> (csrc/icp_fit.hip, LOCGPU_PLANE_DEDUP=1, the default) against icp_plane_accum_kernel<FIT, false>
(LOCGPU_PLANE_DEDUP=0): one plane fit per run of equal neighbour sets must give the bits of a fit per point. The switch is read once per
process, so both settings run tests/gpu_plane_dedup_case.py in a child process each, once for the module, on the same inputs; every
test compares a part of the two results with array_equal (NaN equal to NaN where a non-finite source point reaches the sums).

The inputs. A map of a few thousand points: a ground patch and two walls with 1 cm noise, and two isolated clusters above them. The
designed scan repeats source points to get identical consecutive queries:

    [0, 2048)     runs of 1, 2, 3, 63, 64, 65, 255, 257 and 1100 equal points back to back — they cross lanes 63/0 (6..68), the
                  256-point pp boundary (198..452, 453..709) and the 1024-point block boundary of the four-points-per-thread rung
                  (710..1809) — then single points
    [2048, 4096)  no duplicates: every point is a leader, the plane table of the block is full at every rung (256, 512, 1024 rows)
    [4096, 5120)  256 pairs, then 512 single points: 768 leaders in 1024 points — three full fit passes and a fourth that every
                  wave skips at four points per thread; at two, a block of 256 leaders and a block of singles
    [5120, …)     q1, q2 on opposite sides of a five-point cluster (the same set in another distance order: one plane for both);
                  r1, r2 whose lists differ in the fifth neighbour only (two planes); both pairs checked through the oracle's knn on
                  the CPU; then the run lengths again in falling order, at other offsets

It runs as one scan and as a shared batch of 90 and 179 entries (23 blocks each: icp_accum_split takes 1, 2 and 4 points per thread).
The ragged batch holds counts of 1, 63, 65, 1023, 1025 and 2049 (cut from the runs), an empty scan, and a scan with NaN and inf points
inside a run. Points without a list: under P2Plane the search fills all five slots of every query or, against a target of fewer than
five leaves, none for the whole target (a non-finite source point keeps a full list: the search skips such points for P2P alone). So a
no-list point strictly INSIDE a run of full lists cannot be made through the API; what can be made is covered: points past `counts` in
a scan's last block (the ragged counts), and a four-point target, where every point has i < count and no list — no leader, no fit
pass, all rows zero — at 1 and at 4 points per thread (1800 points, alone and as 512 shared entries of 8 blocks).
That two lists with one set in two distance orders get ONE plane rests on sort5 in both kernels (a 9-comparator network, right on all
32 inputs of zeros and ones); this file shows that such a pair exists in the input and that the two kernels agree on it, not the sharing.
The alignments: icp_align_batch of four scans with repeated points, and the same four as one pooled job."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUNS = [1, 2, 3, 63, 64, 65, 255, 257, 1100]
RUNG_ENTRIES = [90, 179]  # x 23 blocks = 2 070 and 4 117 blocks: 2 and 4 points per thread
NOLIST = (1800, 512)  # points (8 blocks) and shared entries (4 096 blocks: 4 points per thread) of the four-point-target case
POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.05, -0.03, 0.02])
CLUSTER_A, CLUSTER_B = np.array([0.0, 0.0, 8.0]), np.array([5.0, 5.0, 8.0])


def _surface(rng, n):
    """n points on the ground patch and the two walls, without noise."""
    k = rng.randint(0, 4, n)
    u, v = rng.uniform(-9.5, 9.5, n), rng.uniform(0.2, 3.8, n)
    w = rng.uniform(-9.5, 9.5, n)
    g = np.stack([u, w, np.zeros(n)], 1)
    wx = np.stack([np.full(n, 10.0), u, v], 1)
    wy = np.stack([u, np.full(n, 10.0), v], 1)
    return np.where((k < 2)[:, None], g, np.where((k == 2)[:, None], wx, wy))


def _map():
    rng = np.random.RandomState(11)
    body = _surface(rng, 6000) + rng.normal(0.0, 0.01, (6000, 3))
    # cluster A: five points, queried from both sides; cluster B: a core of four, e on one side and f on the other
    a = CLUSTER_A + np.array([[0.10, 0.02, 0.003], [-0.08, 0.07, -0.004], [0.01, -0.11, 0.002], [-0.03, 0.01, 0.006], [0.06, 0.09, -0.005]])
    b = CLUSTER_B + np.array([[0.04, 0.03, 0.002], [-0.05, 0.02, -0.003], [0.01, -0.05, 0.004], [-0.02, 0.04, -0.002], [0.5, 0.0, 0.001], [-0.5, 0.0, -0.001]])
    return np.concatenate([body, a, b]).astype(np.float32)


def _queries(rng, n):
    """n distinct source points that land within a few centimetres of the map's surfaces under POSE."""
    return (_surface(rng, n) + rng.normal(0.0, 0.02, (n, 3)) - POSE[4:]).astype(np.float32)


def _runs(rng, lengths):
    pts = _queries(rng, len(lengths))
    return np.concatenate([np.repeat(pts[i:i + 1], n, axis=0) for i, n in enumerate(lengths)])


def _scan():
    rng = np.random.RandomState(12)
    head = _runs(rng, RUNS)
    assert len(head) == 1810
    head = np.concatenate([head, _queries(rng, 2048 - len(head))])
    nodup = _queries(rng, 2048)
    at_threshold = np.concatenate([_runs(rng, [2] * 256), _queries(rng, 512)])
    t = POSE[4:]
    pairs = np.array([CLUSTER_A + [0.3, 0.0, 0.05] - t, CLUSTER_A + [-0.3, 0.0, 0.05] - t,
                      CLUSTER_B + [0.1, 0.0, 0.02] - t, CLUSTER_B + [-0.1, 0.0, 0.02] - t], dtype=np.float32)
    lead_in = _queries(rng, 37)  # the pairs sit inside a wave, not at its lane 0
    tail = _runs(rng, RUNS[::-1][1:])
    s = np.concatenate([head, nodup, at_threshold, lead_in, pairs, tail])
    return s, 5120 + len(lead_in)


def _inputs():
    m = _map()
    scan, at_pairs = _scan()
    assert -(-len(scan) // 256) == 23
    rng = np.random.RandomState(13)
    ragged = [scan[198:198 + n] for n in (1, 63, 65, 1023, 1025, 2049)] + [scan[:0]]
    hostile = np.repeat(_queries(rng, 1), 100, axis=0)
    hostile[10] = (np.nan, 1.0, 2.0)
    hostile[40] = (np.inf, 0.0, 0.0)
    hostile[41] = (0.0, -np.inf, 1.0)
    ragged.append(hostile)
    align = []
    for i in range(4):
        reps = rng.randint(1, 5, 500 + 37 * i)
        align.append(_runs(rng, reps.tolist()))
    init = POSE + np.array([0, 0, 0, 0, 0.08, -0.06, 0.04])
    return dict(map=m, scan=scan, at_pairs=at_pairs, ragged=ragged, align=align, init=init)


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def results(tmp_path_factory, inputs):
    """{setting: the child's .npz} for LOCGPU_PLANE_DEDUP = "1" and "0"."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("plane_dedup")
    fin = str(tmp / "in.npz")
    blob = dict(nolist_points=NOLIST[0], nolist_entries=NOLIST[1], map=inputs["map"], scan=inputs["scan"], pose=POSE, init=inputs["init"], rung_entries=np.array(RUNG_ENTRIES), n_ragged=len(inputs["ragged"]))
    blob.update({"ragged_%d" % i: s for i, s in enumerate(inputs["ragged"])})
    blob.update({"align_%d" % i: s for i, s in enumerate(inputs["align"])})
    np.savez(fin, **blob)
    out = {}
    for setting in ("1", "0"):
        fout = str(tmp / ("out%s.npz" % setting))
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_plane_dedup_case.py"), fin, fout],
                           env=dict(os.environ, LOCGPU_PLANE_DEDUP=setting), capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[setting] = dict(np.load(fout))
    return out


def _same(results, key):
    on, off = results["1"][key], results["0"][key]
    assert on.shape == off.shape
    return on, off


def test_the_designed_pairs_are_what_they_claim(locref, inputs):
    """The oracle's knn (k = 5, approximate, alpha 0.1) on the CPU: q1 and q2 get one set in two distance orders, r1 and r2 lists that
    differ in the fifth neighbour alone; the repeated points of a run get one list, and the no-duplicate stretch no two equal sets in
    a row."""
    tree = locref.KdTree(inputs["map"])
    scan, at = inputs["scan"], inputs["at_pairs"]
    nn = tree.knn((scan[:, :3].astype(np.float64) + POSE[4:]).astype(np.float32), k=5, approximate=True, alpha=0.1)
    q1, q2, r1, r2 = nn[at:at + 4]
    n_body = len(inputs["map"]) - 11
    assert sorted(q1) == sorted(q2) == list(range(n_body, n_body + 5)) and list(q1) != list(q2)
    assert list(r1[:4]) == list(r2[:4]) or sorted(r1[:4]) == sorted(r2[:4])
    assert len(set(r1) & set(r2)) == 4 and r1[4] != r2[4]
    srt = np.sort(nn, axis=1)
    same_as_prev = (srt[1:] == srt[:-1]).all(axis=1)
    assert same_as_prev[:1809][np.diff(np.repeat(np.arange(len(RUNS)), RUNS)) == 0].all()
    assert not same_as_prev[2048:4095].any()
    assert same_as_prev[4096:4607:2].all() and not same_as_prev[4097:4607:2].any() and not same_as_prev[4607:5119].any()
    print("share of points with the set of the point before them: %.3f" % same_as_prev.mean())


def test_hb_of_the_designed_scan_at_every_rung(results, inputs):
    on, off = _same(results, "hb_single")
    assert np.array_equal(on, off)
    assert on[0] == 1.0 and on[43] > 0.9 * len(inputs["scan"])  # ok, and nearly every point has a fitted plane
    print("one scan: effective_num %d of %d points" % (on[43], len(inputs["scan"])))
    for n in RUNG_ENTRIES:
        on, off = _same(results, "hb_x%d" % n)
        assert on.shape == (n, 44) and np.isfinite(on).all()
        assert np.array_equal(on, off)
        assert (on == on[0]).all() and on[0, 42] == results["1"]["hb_single"][43]


def test_hb_of_the_ragged_batch(results, inputs):
    on, off = _same(results, "hb_ragged")
    counts = [len(s) for s in inputs["ragged"]]
    assert on.shape == (len(counts), 44)
    assert np.array_equal(on, off, equal_nan=True) and on.tobytes() == off.tobytes()
    assert np.isfinite(on[:7]).all() and not on[6].any()  # the empty scan: exactly nothing
    assert on[:6, 42].tolist() == [float(c) for c in counts[:6]]  # every point of the cut runs has a fitted plane
    # the non-finite points keep their lists and planes (effective_num counts them) and poison the sums on both sides alike
    assert on[7, 42] == 100.0 and np.isnan(on[7, :36]).any()
    print("ragged: effective_num %s for counts %s" % (on[:, 42].astype(int).tolist(), counts))


def test_a_target_without_lists(results):
    """Four map points: no query has a list. Nothing is fitted, counted or summed, with either kernel, at 1 and 4 points per thread."""
    on, off = _same(results, "hb_nolist_single")
    assert np.array_equal(on, off) and not on.any()  # ok False, H and B zero, effective_num 0
    on, off = _same(results, "hb_nolist_x")
    assert on.shape == (NOLIST[1], 44) and np.array_equal(on, off) and not on.any()
    assert (on[:, 42] == 0).all()


def test_alignments_of_a_batch_and_of_a_pooled_job(results):
    for kind in ("batch", "pool"):
        p_on, p_off = _same(results, kind + "_poses")
        s_on, s_off = _same(results, kind + "_stats")
        print("%s: iterations %s, converged %s, status %s" % (kind, s_on[:, 0].tolist(), s_on[:, 1].tolist(), s_on[:, 2].tolist()))
        assert np.array_equal(p_on, p_off) and np.array_equal(s_on, s_off)
        assert np.isfinite(p_on).all() and (s_on[:, 0] >= 2).all() and (s_on[:, 2] == 0).all()
    assert np.array_equal(results["1"]["batch_poses"], results["1"]["pool_poses"])  # the pool splits the sums as the plain batch does
