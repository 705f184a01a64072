"""The first descent of the 64-lane walk kernel (walk_descend, csrc/search_walk.hpp): its wave-shared scalar prefix — one node fetch per
level for the whole wave while every lane takes the same turn — the per-lane levels behind it, and the node references the traversal
carries (byte offsets: the sentinel leaf `dummy`, the ids of the result set, kInvalidSlot). The neighbour lists, read back through
locgpu_debug_batch_nn, must equal the oracle's KdTree::GetClosestPoint lists index for index (array_equal, ANN, alpha = 0.1), k = 5
and k = 1. Every batch takes the 64-lane route (more than 2 048 walk waves), asserted through locgpu_debug_batch_run_flags, which has
flags only on that route. The pose is the identity, so a query is its scan point to the bit and the cases below can be designed and
checked on the CPU against the oracle's own tree (KdTree.dump, preorder).

  copies     map of 40 000 points (depth > 13: un-stored levels, T > 0); every wave holds 64 copies of one point — all lanes agree at
             every level, the prefix runs as far as it can
  straddle   same map; the lanes of every wave lie on both sides of the root's split — the lanes part at level 0, the prefix runs zero
             levels
  tiny1/2/5/64  maps of 1, 2, 5 and 64 points — T = 0, no prefix, a leaf at the root or just below; lists shorter than k (a map of
             fewer than five points gives its points in distance order, then -1)
  lines      four straight lines with geometric spacing (ratio 2.5, 36 points each): the mean split peels a few points off per level —
             depth 26, T = 13, with leaves on levels 4 … 11. One wave of 64 copies per such leaf: the prefix meets a LEAF. Asserted on
             the oracle's tree: such leaves exist and those queries' descents end on them.
  ragged     counts 64 k + 1 and 64 k − 1, 1, 63 and 65 among full scans: a wave with one live lane, waves wholly past the count
  LOCGPU_FAST_STACK = 12, 15, 24 (a process each): copies, straddle and ragged again with plain stored rows instead of the window —
             the other descent loops behind the prefix."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
WAVES = 58          # 3 712 points per scan
ENTRIES = 36        # 36 x 58 = 2 088 waves > 2 048
STACKS = ("12", "15", "24")
BIG = ("copies", "straddle", "ragged")
TINY = (1, 2, 5, 64)


def _tree_levels(axis):
    """(level, right child) per node of a preorder dump (left subtree first; axis < 0 = leaf); the left child of node i is i + 1."""
    n = len(axis)
    level = np.zeros(n, dtype=np.int64)
    right = np.full(n, -1, dtype=np.int64)
    pending = []  # (parent, is right child) of the nodes still to come, innermost last
    for i in range(n):
        if i:
            parent, is_right = pending.pop()
            level[i] = level[parent] + 1
            if is_right:
                right[parent] = i
        if axis[i] >= 0:
            pending.append((i, True))
            pending.append((i, False))
    return level, right


def _descend(axis, th, right, q):
    """Node index of the leaf the first descent of float32 query q ends on (KdTree::Knn: left when q[axis] < thresh)."""
    i = 0
    while axis[i] >= 0:
        i = i + 1 if q[axis[i]] < th[i] else int(right[i])
    return i


def _lines_map():
    rng = np.random.default_rng(4)
    d = rng.normal(size=(4, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = rng.uniform(-1, 1, size=(4, 3))
    t = 0.001 * 2.5 ** np.arange(36)
    return (o[:, None, :] + t[None, :, None] * d[:, None, :]).reshape(-1, 3).astype(np.float32)


def _inputs(locref):
    rng = np.random.default_rng(11)
    d, info = {"pose": POSE}, {}
    big = rng.uniform(-40, 40, size=(40000, 3)).astype(np.float32)
    tree = locref.KdTree(big)
    axis, th, _ = tree.dump()
    info["big_depth"] = tree.depth
    near = lambda n: (big[rng.integers(0, len(big), n)] + rng.normal(0, 0.3, size=(n, 3))).astype(np.float32)  # noqa: E731
    # copies: 58 points, 64 times each
    d["map_copies"], d["scan_copies"], d["entries_copies"] = big, np.repeat(near(WAVES), 64, axis=0), ENTRIES
    # straddle: the root's axis coordinate alternates between just below and just above the root's threshold
    s = near(WAVES * 64)
    s[:, axis[0]] = th[0] + np.where(np.arange(len(s)) % 2 == 0, -1.0, 1.0).astype(np.float32) * rng.uniform(0.01, 2.0, len(s)).astype(np.float32)
    d["map_straddle"], d["scan_straddle"], d["entries_straddle"] = big, s, ENTRIES
    info["straddle_left"] = (s[:, axis[0]] < th[0]).reshape(WAVES, 64)
    # ragged: max 3 713 points = 59 waves, 36 scans
    counts = [64 * WAVES + 1, 64 * WAVES - 1, 1, 63, 65] + [64 * WAVES + 1] * (ENTRIES - 5)
    full = near(64 * WAVES + 1)
    d["map_ragged"], d["n_ragged_ragged"] = big, len(counts)
    for i, c in enumerate(counts):
        d["ragged_ragged_%d" % i] = full[:c] if i >= 5 else near(c)
    info["ragged_counts"] = counts
    # tiny maps
    for n in TINY:
        c = "tiny%d" % n
        d["map_" + c] = rng.uniform(-5, 5, size=(n, 3)).astype(np.float32)
        d["scan_" + c], d["entries_" + c] = rng.uniform(-8, 8, size=(WAVES * 64, 3)).astype(np.float32), ENTRIES
    # lines: one wave of copies per leaf that lies above the un-stored levels' end, then six waves of points near the map
    lines = _lines_map()
    lt = locref.KdTree(lines)
    laxis, lth, lpidx = lt.dump()
    level, right = _tree_levels(laxis)
    T = lt.depth - 13  # the window shape leaves the levels above depth − 13 un-stored (icp_search.hip, kWindowStored); depth counts levels
    shallow = np.flatnonzero((laxis < 0) & (level < T - 1))
    at = lines[lpidx[shallow]]
    jit = (lines[rng.integers(0, len(lines), 6 * 64)] * (1.0 + rng.normal(0, 0.05, size=(6 * 64, 3)))).astype(np.float32)
    d["map_lines"], d["scan_lines"] = lines, np.concatenate([np.repeat(at, 64, axis=0), jit])
    d["entries_lines"] = -(-2049 // (len(d["scan_lines"]) // 64))
    info.update(lines_depth=lt.depth, lines_T=T, lines_shallow=shallow, lines_level=level,
                lines_reached=np.array([_descend(laxis, lth, right, q) for q in at]))
    return d, info


def _want(locref, cloud, scan, k):
    if k > len(cloud):  # fewer points than k: the points in distance order, then nothing (GetClosestPoint itself refuses k > size)
        return np.concatenate([locref.KdTree(cloud).knn(scan, len(cloud), approximate=True, alpha=0.1), np.full((len(scan), k - len(cloud)), -1, np.int32)], axis=1)
    return locref.KdTree(cloud).knn(scan, k, approximate=True, alpha=0.1)


@pytest.fixture(scope="module")
def world(locref, tmp_path_factory):
    """(inputs, CPU-side facts, oracle lists {(case, k)}, child results {stack setting or "": npz})."""
    d, info = _inputs(locref)
    want = {}
    for c in ("copies", "straddle", "lines") + tuple("tiny%d" % n for n in TINY):
        for k in (5, 1):
            want[c, k] = _want(locref, d["map_" + c], d["scan_" + c], k)
    for k in (5, 1):
        want["ragged", k] = [_want(locref, d["map_ragged"], d["ragged_ragged_%d" % i], k) for i in range(len(info["ragged_counts"]))]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("walk_prefix")
    fin = str(tmp / "in.npz")
    np.savez(fin, **d)
    every = ",".join(BIG + ("lines",) + tuple("tiny%d" % n for n in TINY))
    out = {}
    for stack, cases in [("", every)] + [(s, ",".join(BIG)) for s in STACKS]:
        fout = str(tmp / ("out_%s.npz" % stack))
        env = dict(os.environ)
        env.pop("LOCGPU_FAST_STACK", None)
        if stack:
            env["LOCGPU_FAST_STACK"] = stack
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_walk_prefix_case.py"), fin, fout, cases], env=env, capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[stack] = dict(np.load(fout))
    return d, info, want, out


def _check_shared(world, case, stack=""):
    d, _, want, out = world
    res, n = out[stack], len(d["scan_" + case])
    assert res["written_" + case], "not the 64-lane route"
    for k in (5, 1):
        got = res["nn%d_%s" % (k, case)]
        assert got.shape == (2, n, k) and res["same%d_%s" % (k, case)]
        for e in (0, 1):
            assert np.array_equal(got[e], want[case, k]), (case, stack, k, e, int(np.sum(np.any(got[e] != want[case, k], axis=1))))


def _check_ragged(world, stack=""):
    _, info, want, out = world
    res, counts = out[stack], info["ragged_counts"]
    assert res["written_ragged"], "not the 64-lane route"
    assert len(counts) * ((max(counts) + 63) // 64) > 2048
    for k in (5, 1):
        got = res["nn%d_ragged" % k]
        assert got.shape == (len(counts), max(counts), k)
        for i, c in enumerate(counts):
            assert np.array_equal(got[i, :c], want["ragged", k][i]), (stack, k, i, c)
            assert (got[i, c:] == -1).all()


def test_all_lanes_of_a_wave_agree_down_to_the_leaf(world):
    d, info, _, _ = world
    assert info["big_depth"] > 13  # un-stored levels exist: T > 0
    assert (d["scan_copies"].reshape(WAVES, 64, 3) == d["scan_copies"].reshape(WAVES, 64, 3)[:, :1]).all()
    _check_shared(world, "copies")


def test_lanes_part_at_the_root(world):
    _, info, _, _ = world
    left = info["straddle_left"]
    assert left.any(axis=1).all() and (~left).any(axis=1).all()  # every wave has lanes on both sides of the root's split
    _check_shared(world, "straddle")


@pytest.mark.parametrize("n", TINY)
def test_maps_of_a_few_points(world, n):
    d, _, _, out = world
    _check_shared(world, "tiny%d" % n)
    got = out[""]["nn5_tiny%d" % n][0]
    assert ((got >= 0).sum(axis=1) == min(n, 5)).all() and (got[:, min(n, 5):] == -1).all()


def test_a_leaf_inside_the_shared_prefix(world):
    d, info, _, _ = world
    shallow, level, T = info["lines_shallow"], info["lines_level"], info["lines_T"]
    print("lines map: depth %d, T %d, %d leaves on levels %s" % (info["lines_depth"], T, len(shallow), sorted(set(level[shallow].tolist()))))
    assert T > 2 and len(shallow) >= 16 and (level[shallow] < T - 1).all()  # leaves above level T exist, with a level to spare
    assert np.array_equal(info["lines_reached"], shallow)  # … and the designed queries' descents end on them, a whole wave each
    assert d["entries_lines"] * (len(d["scan_lines"]) // 64) > 2048
    _check_shared(world, "lines")


def test_ragged_counts(world):
    _check_ragged(world)


@pytest.mark.parametrize("stack", STACKS)
def test_plain_stored_rows_behind_the_prefix(world, stack):
    _check_shared(world, "copies", stack)
    _check_shared(world, "straddle", stack)
    _check_ragged(world, stack)
