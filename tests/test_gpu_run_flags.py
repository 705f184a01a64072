"""The run flags of the search stage (icp_search_walk_kernel<5, ·, 64, ·, ·>, csrc/icp_search.hip) and the plane kernel that takes
its runs from them (plane_accum_flagged, csrc/icp_fit.hip; LOCGPU_PLANE_RUNFLAGS=1, the default) against the plane kernel that finds
the runs itself (LOCGPU_PLANE_RUNFLAGS=0): the bits must be the same. The switch is read once per process, so both settings run
tests/gpu_run_flags_case.py in a child process each, once for the module, on the same inputs.

A. Bits (array_equal on H/B, poses and statistics), on inputs that take the 64-lane walk kernel (more than 2 048 walk waves):
   the designed scan of test_gpu_plane_dedup.py (runs of 1 … 1100 equal points across lane, 256- and 1 024-point boundaries) as
   shared batches of 90 and 179 entries (2 and 4 points per thread) and 33 entries of its first 4 000 points (63 waves each: 2 079
   waves, 528 blocks, 1 point per thread); alone (16-lane kernel: no flags, the fall-back); the ragged batch (counts 1, 63, 64, 65,
   1023, 1025, 2049, an empty scan, NaN / inf points inside a run) padded with 60 scans of 2 049 points (68 × 33 = 2 244 waves); the
   four-point target (no point has a list: all leaders, none fits); a lattice map (ties: in-wave exact walk, redo kernel); a far pose
   under LOCGPU_FAST_STACK=12 against a 60 000-point map with the lattice beside it (deep pass and ties common, the runs of the
   designed scan and of the lattice scan among them); icp_align_batch of 40 scans of repeated points (52+ waves each), the same as one pooled job, the batch under
   graph capture, and the grid search (no flags).
   Pairs of points 5 cm apart over a 120-point map (33 entries of 4 000 points): one set in two distance orders follows.
B. The flags themselves (locgpu_debug_batch_run_flags against locgpu_debug_batch_nn after one search stage): a follower is never lane
   0, has a full list and the set of the point before it (exact); flagged leaders exceed the exact ones (tests/run_flags_ref.py) by at
   most 2 × (queries sent to the deep pass + queries answered exactly): each such query makes itself and the point behind it a leader."""
import os
import subprocess
import sys

import numpy as np
import pytest

from run_flags_ref import leaders, unpack_flags
from test_gpu_plane_dedup import POSE, RUNS, _map, _scan, _surface

pytestmark = pytest.mark.gpu

NOLIST = (1800, 512)  # points (29 waves, 8 blocks) and shared entries (4 096 blocks: 4 points per thread) of the four-point-target case
N_ALIGN = 40


def _inputs():
    m = _map()
    scan, _ = _scan()
    rng = np.random.RandomState(21)
    ragged = [scan[198:198 + n] for n in (1, 63, 64, 65, 1023, 1025, 2049)] + [scan[:0]]
    hostile = np.repeat((_surface(rng, 1) - POSE[4:]).astype(np.float32), 100, axis=0)
    hostile[10] = (np.nan, 1.0, 2.0)
    hostile[40] = (np.inf, 0.0, 0.0)
    hostile[41] = (0.0, -np.inf, 1.0)
    ragged.append(hostile)
    n_named = len(ragged)
    ragged += [scan[198:198 + 2049]] * 60
    assert len(ragged) * ((2049 + 63) // 64) > 2048
    align = []
    for i in range(N_ALIGN):
        pts = (_surface(rng, 1400 + 7 * i) + rng.normal(0.0, 0.02, (1400 + 7 * i, 3)) - POSE[4:]).astype(np.float32)
        align.append(np.repeat(pts, rng.randint(1, 5, len(pts)), axis=0))
    assert N_ALIGN * ((max(len(s) for s in align) + 63) // 64) > 2048
    # initial poses 0.1 to 1 m and 0 to 8 degrees of yaw off: the scans finish at different iterations, some of them in a later chunk
    inits = []
    for i in range(N_ALIGN):
        yaw = np.deg2rad(2.0 * (i % 5))
        inits.append(np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2), *(POSE[4:] + np.array([0.08, -0.06, 0.04]) * (1 + 2 * (i % 5)))]))
    inits = np.stack(inits)
    # lattice map; the scan: runs of 1-3 equal points, on map points (zero distances, ties everywhere) and beside them, interleaved
    g = np.arange(-12, 13, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g[:6], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    # (a point beside a lattice point follows the query ON that point: five of the same seven neighbours, often the same five)
    on = lattice[rng.choice(len(lattice), 1500)]
    beside = (on + rng.normal(0, 0.05, (1500, 3))).astype(np.float32)
    mixed = np.stack([on, beside], axis=1).reshape(-1, 3)
    lattice_scan = np.repeat(mixed, rng.randint(1, 4, len(mixed)), axis=0)
    assert 40 * ((len(lattice_scan) + 63) // 64) > 2048
    lattice_pose = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])  # the identity: the on-map queries stay on the map
    # far case: 60 000 surface points and, below the ground, the lattice; the designed scan and the lattice scan under a pose metres
    # off — a translation by whole metres, which keeps the on-lattice queries on the lattice to the bit, so their distances tie
    body = (_surface(rng, 60000) + rng.normal(0.0, 0.01, (60000, 3))).astype(np.float32)
    far_map = np.concatenate([body, lattice])
    far_pose = np.array([0.0, 0.0, 0.0, 1.0, 2.0, -1.0, 1.0])
    far_scan = np.concatenate([scan, (lattice_scan - far_pose[4:]).astype(np.float32)])
    # pairs 5 cm apart over a map of 120 points
    small_map = (_surface(rng, 120) + rng.normal(0.0, 0.01, (120, 3))).astype(np.float32)
    base = _surface(rng, 2000) + rng.normal(0.0, 0.02, (2000, 3)) - POSE[4:]
    order_scan = np.stack([base, base + rng.normal(0.0, 0.05, (2000, 3))], axis=1).reshape(-1, 3).astype(np.float32)
    assert 33 * ((len(order_scan) + 63) // 64) > 2048
    return dict(map=m, scan=scan, small_map=small_map, order_scan=order_scan, ragged=ragged, n_named=n_named, align=align, inits=inits, lattice=lattice, lattice_scan=lattice_scan,
                lattice_pose=lattice_pose, far_map=far_map, far_pose=far_pose, far_scan=far_scan)


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def results(tmp_path_factory, inputs):
    """{(case, setting): the child's .npz} for case "main" / "far" and LOCGPU_PLANE_RUNFLAGS = "1" / "0"."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("run_flags")
    fin = str(tmp / "in.npz")
    blob = {k: inputs[k] for k in ("map", "scan", "inits", "lattice", "lattice_scan", "lattice_pose", "far_map", "far_pose", "far_scan", "small_map", "order_scan")}
    blob.update(pose=POSE, nolist_points=NOLIST[0], nolist_entries=NOLIST[1], n_ragged=len(inputs["ragged"]), n_align=N_ALIGN)
    blob.update({"ragged_%d" % i: s for i, s in enumerate(inputs["ragged"])})
    blob.update({"align_%d" % i: s for i, s in enumerate(inputs["align"])})
    np.savez(fin, **blob)
    out = {}
    for case, extra in (("main", {}), ("far", {"LOCGPU_FAST_STACK": "12"})):
        for setting in ("1", "0"):
            fout = str(tmp / ("out_%s_%s.npz" % (case, setting)))
            r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_run_flags_case.py"), fin, fout, case],
                               env=dict(os.environ, LOCGPU_PLANE_RUNFLAGS=setting, **extra), capture_output=True, text=True, timeout=300, cwd=root)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            out[case, setting] = dict(np.load(fout))
    return out


def _same(results, key, case="main"):
    on, off = results[case, "1"][key], results[case, "0"][key]
    assert on.shape == off.shape
    return on, off


# ------------------------------------------------------------------------------------------------------------------- A. bits
def test_which_stages_wrote_flags(results):
    on, off = results["main", "1"], results["main", "0"]
    for key in ("x90", "x179", "x33", "ragged", "lattice", "nolist_x90", "nolist_x"):
        assert on["written_" + key] and not off["written_" + key], key
    for key in ("single", "grid"):  # the 16-lane kernel and the grid search write none: the plane kernel finds the runs itself
        assert not on["written_" + key] and not off["written_" + key], key
    assert results["far", "1"]["written_far"] and not results["far", "0"]["written_far"]


def test_hb_of_the_designed_scan_at_every_rung(results, inputs):
    on, off = _same(results, "hb_single")
    assert np.array_equal(on, off) and on[0, 43] == 1.0 and on[0, 42] > 0.9 * len(inputs["scan"])
    for key, n in (("x90", 90), ("x179", 179), ("x33", 33), ("grid", 90)):
        on, off = _same(results, "hb_" + key)
        assert on.shape == (n, 44) and np.isfinite(on).all()
        assert np.array_equal(on, off), key
        assert (on == on[0]).all()


def test_hb_of_the_ragged_batch(results, inputs):
    on, off = _same(results, "hb_ragged")
    counts = [len(s) for s in inputs["ragged"]]
    k = inputs["n_named"]
    assert on.shape == (len(counts), 44)
    assert np.array_equal(on, off, equal_nan=True) and on.tobytes() == off.tobytes()
    assert np.isfinite(on[:k - 1]).all() and not on[k - 2].any()  # the empty scan: exactly nothing
    assert on[:k - 2, 42].tolist() == [float(c) for c in counts[:k - 2]]  # every point of the cut runs has a fitted plane
    assert on[k - 1, 42] == 100.0 and np.isnan(on[k - 1, :36]).any()  # the non-finite points keep their lists and planes
    print("ragged: effective_num %s for counts %s" % (on[:k, 42].astype(int).tolist(), counts[:k]))


def test_a_target_without_lists(results):
    """Four map points: no query has a list. Every point is flagged a leader, none fits: nothing is counted or summed."""
    for key, n in (("nolist_x90", 90), ("nolist_x", NOLIST[1])):
        on, off = _same(results, "hb_" + key)
        assert on.shape == (n, 44) and np.array_equal(on, off) and not on.any()
    flags = results["main", "1"]["flags_nolist_x90"]
    assert all(unpack_flags(flags[e], NOLIST[0]).all() for e in range(90))
    assert (results["main", "1"]["nn_nolist_x90"][:, :NOLIST[0], 4] == -1).all()  # four neighbours at the most: no full list


def test_hb_on_a_lattice_map(results, inputs):
    on, off = _same(results, "hb_lattice")
    assert np.array_equal(on, off) and np.isfinite(on).all()
    searched, redone, walked = results["main", "1"]["stats_lattice"]
    print("lattice: %d queries, %d answered exactly, %d through the deep pass" % (searched, redone, walked))
    assert redone > 0.2 * searched  # the input does what it is for: ties are common


def test_hb_at_a_far_pose_with_twelve_stack_rows(results):
    on, off = _same(results, "hb_far", "far")
    assert np.array_equal(on, off) and np.isfinite(on).all()
    searched, redone, walked = results["far", "1"]["stats_far"]
    print("far pose, 12 rows: %d queries, %d answered exactly, %d through the deep pass" % (searched, redone, walked))
    assert walked > 0.01 * searched and redone > 0  # the input does what it is for: the deep pass is common, ties occur


def test_alignments_of_a_batch_a_pooled_job_and_a_captured_graph(results):
    for kind in ("batch", "pool", "graph"):
        p_on, p_off = _same(results, kind + "_poses")
        s_on, s_off = _same(results, kind + "_stats")
        print("%s: iterations %d..%d, converged %d of %d" % (kind, s_on[:, 0].min(), s_on[:, 0].max(), s_on[:, 1].sum(), len(s_on)))
        assert np.array_equal(p_on, p_off) and np.array_equal(s_on, s_off)
        assert np.isfinite(p_on).all() and (s_on[:, 0] >= 2).all() and (s_on[:, 2] == 0).all()
    on = results["main", "1"]
    assert np.array_equal(on["batch_poses"], on["pool_poses"]) and np.array_equal(on["batch_poses"], on["graph_poses"])
    # the inputs do what they are for (eps = 1e-11): scans finish at different iterations, some behind the first chunk of eight —
    # where the launches go over `active` lists, and with few scans left over the 16-lane walk kernel, which writes no flags
    its = on["batch_stats"][:, 0]
    assert its.max() > 8 and len(set(its.tolist())) > 1


# ------------------------------------------------------------------------------------------------------------------- B. the flags
def _check_flags(res, key, n):
    """Safety on every entry; returns (flagged leaders, exact leaders, deep + exact queries) over the batch."""
    flags, nn = res["flags_" + key], res["nn_" + key][:, :n]
    _, redone, walked = res["stats_" + key]
    flagged = exact = 0
    for e in range(len(flags)):
        lead = unpack_flags(flags[e], n)
        fol = np.flatnonzero(~lead)
        assert (fol % 64 != 0).all()
        assert (nn[e, fol] >= 0).all()
        assert np.array_equal(np.sort(nn[e, fol], axis=1), np.sort(nn[e, fol - 1], axis=1))
        want = leaders(nn[e])
        assert not (want & ~lead).any()  # the same statement, from the other side
        flagged += int(lead.sum())
        exact += int(want.sum())
    return flagged, exact, int(redone + walked)


def test_flags_of_the_designed_batch(results, inputs):
    res, n = results["main", "1"], len(inputs["scan"])
    flagged, exact, unknown = _check_flags(res, "x90", n)
    print("designed batch: %d flagged leaders, %d exact leaders, %d deep or exact queries" % (flagged, exact, unknown))
    assert flagged - exact <= 2 * unknown
    flags = res["flags_x90"]
    first = sum(RUNS[:-1])  # the 1100-run is points [710, 1810)
    idx = np.arange(first, first + RUNS[-1])
    want_run = (idx % 64 == 0) | (idx == first)
    extra = 0
    for e in range(90):
        lead = unpack_flags(flags[e], n)
        assert lead[2048:4096].all()  # the no-duplicate stretch: every point leads
        assert lead[idx][want_run].all()
        extra += int((lead[idx] & ~want_run).sum())
    assert extra <= 2 * unknown  # every other point of the 1100-run follows, unless the counters say it went to the deep pass
    if unknown == 0:
        assert flagged == exact


def test_one_set_in_two_distance_orders_follows(results, inputs):
    """Pairs of points 5 cm apart over a 120-point map: the second of a pair mostly has the first one's five neighbours, often in
    another distance order, and must follow it all the same — the walk kernel compares SORTED lists. The tree is seven levels deep:
    no query goes to the deep pass, none ties, so the flagged leaders are the exact ones to the point."""
    res, n = results["main", "1"], len(inputs["order_scan"])
    assert res["written_order"]
    nn = res["nn_order"][0, :n]
    same_set = np.zeros(n, dtype=bool)
    same_set[1:] = (np.sort(nn[1:], axis=1) == np.sort(nn[:-1], axis=1)).all(axis=1)
    other_order = same_set.copy()
    other_order[1:] &= (nn[1:] != nn[:-1]).any(axis=1)
    other_order &= np.arange(n) % 64 != 0
    flagged, exact, unknown = _check_flags(res, "order", n)
    print("pairs: %d of %d points have the previous point's set, %d of them in another order; %d deep or exact queries"
          % (same_set.sum(), n, other_order.sum(), unknown))
    assert other_order.sum() >= 20 and unknown == 0  # the input is what it claims
    assert flagged == exact
    assert not unpack_flags(res["flags_order"][0], n)[other_order].any()


def test_flags_among_ties_and_deep_queries(results, inputs):
    for case, key, n in (("main", "lattice", len(inputs["lattice_scan"])), ("far", "far", len(inputs["far_scan"]))):
        flagged, exact, unknown = _check_flags(results[case, "1"], key, n)
        print("%s: %d flagged leaders, %d exact leaders, %d deep or exact queries" % (key, flagged, exact, unknown))
        assert flagged - exact <= 2 * unknown
