"""The neighbour LISTS of the exact grid stage (search_mode = SEARCH_GRID_EXACT: grid_bin_count_kernel, grid_bin_scatter_kernel,
grid_tile_search_kernel, then icp_search_walk_list_kernel for what is left — csrc/grid_kernels.hip) against the oracle's exact k-NN,
index for index, on inputs designed to reach one path of the stage each (tests/grid_list_cases.py; tests/test_grid_route_ref.py shows
on the CPU that they do).

Every case: set the target, build a batch, read the search counters once to switch them on, icp_hb_batch in grid mode for P2Plane
(k = 5) and P2P (k = 1), read the lists back with debug_batch_nn and compare every row below the scan's count with
locref.KdTree(map).knn(q32, k, approximate=False), q32 the float32 of the pose applied to the scan. There is no helper that forgives
ties: the stage hands ties to the tree so that they come out as the oracle has them. Then the counters. In grid mode `searched` counts
the queries grid_bin_count_kernel looked at (all but the non-finite points P2P skips) and `walked` the length of the list
icp_search_walk_list_kernel got, i.e. what the bin kernel and the tile kernel handed to the tree. Three things hold for all cases:

  bounds        walked ≥ outside + no_tile + no_fit as grid_route_ref.route() counts them on the DUMPED grid (integer decisions; the
                tile kernel cannot answer those). route() follows settle_top in float32 as well, so the test holds `walked` between
                that sum + open + tie and the same + may_tie (queries with two equal distances among their candidates, which
                TopK's wider tie test may or may not flag): a stage that sends MORE to the tree than its rules say — a face
                taken for open that is not, a slack too large — gives right lists and shows here only.
  cap           walked / searched ≤ the case's cap: what keeps a case from passing by the tree fallback alone. A condition on the
                input, not a tolerance.
  bits          H/B of the same batch under search_mode = TREE, approximate = 0 has the same bytes: the fit stage reads nothing but
                the lists.

Each case prints searched, walked, the route() classes and the cap.

Mutations of grid_kernels.hip tried against this file in scratch builds, one rebuild and one run each, with
test_icp_grid_mode_matches_exact_oracle and the grid tests of test_gpu_configs.py beside it (neither of the latter failed unless said):
  settle_top `cx + R < nx - 1` -> `<=`   sparse_half, sparse_offset (lists right; `walked` above route()'s upper bound)
  slack = 0                               sparse_offset (`walked` below the lower bound)
  TopK::finish() returns false            line, ties, ties_flat
  ring-2 loop over 24 rows                sparse_tilted (the flat sparse_half cannot see it: its rows with dz != 0 are empty)
  s_lstart[id0 + 3] -> + 2 in ring 1      every case with a list, and test_icp_grid_mode_matches_exact_oracle
  fits always true (staging clamped)      clump, ties
  (j + 2) / 4 -> (j + 1) / 4 in staging   every case, and test_icp_grid_mode_matches_exact_oracle
  rank dropped in the scatter kernel      room, sheet, line; the run then stopped at its time limit in `wide` — a property of the
                                          mutant (it leaves most of `sorted` unwritten), not looked into and not repeated"""
import numpy as np
import pytest

import grid_list_cases as C
import grid_route_ref as R

pytestmark = pytest.mark.gpu

METHODS = ((2, 5), (0, 1))  # (P2PLANE, k = 5), (P2P, k = 1)


@pytest.fixture(scope="module")
def ctx(api):
    """A context of this file's own: the search counters stay on once they were read."""
    api.lib()
    c = api.Context(0)
    yield c
    c.close()


def q32_of(locref, scan, pose):
    return locref.transform_points(pose, np.ascontiguousarray(scan[:, :3], dtype=np.float64)).astype(np.float32)


def grid_opts(api, method, **kw):
    return api.icp_opts(method=method, search_mode=api.SEARCH_GRID_EXACT, **kw)


def tree_opts(api, method, **kw):
    return api.icp_opts(method=method, approximate=0, **kw)


def check_lists(got, want, what):
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d lists differ from the oracle's, first at row %d: got %s want %s" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def run_batch(api, locref, ctx, tree, grid, scans, poses, what, cap=None, tie_bound=False, shared=None):
    """Grid-mode lists of every scan of one batch against the oracle, counters against route(), H/B bytes against exact tree mode.
    Returns {k: (lists [n_scans, max_points, k], stats)}."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    b = ctx.batch_shared(shared, len(poses)) if shared is not None else ctx.batch(scans)
    if shared is not None:
        scans = [shared] * len(poses)
    out = {}
    try:
        ctx.search_stats_read(reset=True)  # switches the counters on and zeroes them
        q32 = [q32_of(locref, s, p) if len(s) else np.zeros((0, 3), np.float32) for s, p in zip(scans, poses)]
        for method, k in METHODS:
            hb_grid = ctx.icp_hb_batch(b, poses, grid_opts(api, method))
            nn = ctx.debug_batch_nn(b, k)
            st = ctx.search_stats_read(reset=True)
            routed = [R.route(grid, q, k, detail=True) for q in q32]
            cls, may_tie = np.concatenate([r[0] for r in routed]), np.concatenate([r[1] for r in routed])
            sure = R.to_tree_for_sure(cls) + (int(np.sum(cls == "tie")) if tie_bound else 0)
            least, most = R.walked_bounds(cls, may_tie)
            n_all = sum(len(s) for s in scans)
            print("%s k=%d: searched %d walked %d (%.2f%%) | route: %s | walked between %d and %d, cap %s" % (
                what, k, st["searched"], st["walked"], 100.0 * st["walked"] / max(st["searched"], 1), R.fmt(cls), least, most, "none" if cap is None else "%.0f%%" % (100 * cap)))
            for i, (s, q) in enumerate(zip(scans, q32)):
                assert np.all(nn[i, len(s):] == -1), what  # rows past the scan's count: not lists
                if len(s) == 0:
                    continue
                if k > tree.num_leaves:  # the oracle returns nothing; the product leaves the k-th slot empty (locgpu_api.hip: check_icp)
                    assert np.all(nn[i, :len(s), k - 1] == -1), what
                else:
                    check_lists(nn[i, :len(s)], tree.knn(q, k, approximate=False), "%s scan %d k=%d" % (what, i, k))
            assert st["searched"] == n_all, (what, k, st, n_all)
            assert st["walked"] >= sure, (what, k, st, R.fmt(cls))
            assert least <= st["walked"] <= most, (what, k, st, R.fmt(cls), least, most)
            if cap is not None:
                assert st["walked"] <= cap * st["searched"], (what, k, st, R.fmt(cls))
            hb_tree = ctx.icp_hb_batch(b, poses, tree_opts(api, method))
            ctx.search_stats_read(reset=True)
            assert hb_grid.tobytes() == hb_tree.tobytes(), "%s k=%d: H/B of grid mode and of exact tree mode differ by %.3g" % (what, k, np.nanmax(np.abs(hb_grid - hb_tree)))
            out[k] = (nn, st)
    finally:
        b.close()
    return out


def set_target(api, locref, ctx, m, same_as_ladder=True):
    ctx.icp_set_target(m)
    grid = R.grid_dump(api, ctx)
    tree = locref.KdTree(m)
    assert grid["n"] == tree.num_leaves
    if same_as_ladder:  # what the CPU test showed about the input holds for the grid the library built
        lad = R.ladder(m)
        assert list(grid["dims"]) == list(lad["dims"]) and grid["cell"] == lad["cell"] and grid["n_tocc"] == lad["n_tocc"], (grid["dims"], grid["cell"], lad["dims"], lad["cell"])
        assert abs(float(grid["slack"]) - float(lad["slack"])) <= 1e-6 * float(lad["slack"])
    return grid, tree


@pytest.mark.parametrize("make", C.SINGLE, ids=[m.__name__ for m in C.SINGLE])
def test_designed_scan(api, locref, ctx, make):
    c = make()
    grid, tree = set_target(api, locref, ctx, c["map"])
    out = run_batch(api, locref, ctx, tree, grid, [c["scan"]], [c["pose"]], c["name"], cap=c["cap"], tie_bound=c.get("tie_bound", False))
    q = q32_of(locref, c["scan"], c["pose"])
    if c["name"] == "sparse_half":  # on the dumped grid: at least half of the k = 5 queries need the 5×5×5 shell
        assert np.mean(R.route(grid, q, 5) == "ring2") >= c["ring2_share"]
    if c["name"] == "clump":
        assert np.mean(R.route(grid, q, 5) == "no_fit") >= c["no_fit_share"]
    if c["name"] == "room_edges":
        assert out[5][1]["walked"] >= c["n_outside_min"]


@pytest.mark.parametrize("name", [t[0] for t in C.tiny_targets()])
def test_tiny_targets(api, locref, ctx, name):
    """Targets of 1, 4, 5, 6 and 12 leaves and one of equal points. With fewer than five leaves the oracle's k = 5 search returns
    nothing; the product shows that by an empty fifth slot (the fit stage reads it), which is what is asserted there, and the H/B bytes
    of grid and tree mode are equal as everywhere."""
    m, q = [(m, q) for n, m, q in C.tiny_targets() if n == name][0]
    grid, tree = set_target(api, locref, ctx, m, same_as_ladder=(name != "all_equal"))
    run_batch(api, locref, ctx, tree, grid, [q], [C.IDENT], name)


def test_ragged_batch(api, locref, ctx):
    """Counts 0, 1, 255, 256, 257 and 2 000 under six poses in one batch: per-scan early-outs and the last block of each scan."""
    m, scans, poses = C.ragged_batch()
    grid, tree = set_target(api, locref, ctx, m)
    run_batch(api, locref, ctx, tree, grid, scans, poses, "ragged", cap=0.02)


def test_more_ranges_than_waves(api, locref, ctx):
    """270 copies of a 2 000-point scan: 2 110 ranges of 256 sorted queries for 2 048 one-wave workgroups, so the grid-stride loop of
    the tile kernel runs; the last copy against the oracle, every copy equal to it."""
    m, scans, poses = C.ragged_batch()
    grid, tree = set_target(api, locref, ctx, m)
    scan, pose = scans[-1], poses[-1]
    assert -(-C.COPIES * len(scan) // R.RANGE_Q) > 2048
    b = ctx.batch([scan] * C.COPIES)
    try:
        ctx.search_stats_read(reset=True)
        q = q32_of(locref, scan, pose)
        for method, k in METHODS:
            P = np.stack([pose] * C.COPIES)
            hb_grid = ctx.icp_hb_batch(b, P, grid_opts(api, method))
            nn = ctx.debug_batch_nn(b, k)
            st = ctx.search_stats_read(reset=True)
            cls = R.route(grid, q, k)
            print("copies k=%d: searched %d walked %d (%.2f%%) | route of one copy: %s | cap 2%%" % (k, st["searched"], st["walked"], 100.0 * st["walked"] / st["searched"], R.fmt(cls)))
            check_lists(nn[-1, :len(scan)], tree.knn(q, k, approximate=False), "last copy k=%d" % k)
            assert np.array_equal(nn[:, :len(scan)], np.broadcast_to(nn[-1, :len(scan)], (C.COPIES, len(scan), k)))
            assert st["searched"] == C.COPIES * len(scan) and st["walked"] >= C.COPIES * R.to_tree_for_sure(cls) and st["walked"] <= 0.02 * st["searched"]
            hb_tree = ctx.icp_hb_batch(b, P, tree_opts(api, method))
            ctx.search_stats_read(reset=True)
            assert hb_grid.tobytes() == hb_tree.tobytes()
    finally:
        b.close()


def test_shared_source_batch(api, locref, ctx):
    """The shared-source form of the init searches (SearchArgs::src_of): two entries that read one resident scan under two poses.
    debug_batch_nn reads such a batch's lists like any other's."""
    m, scan, poses = C.shared_pair()
    grid, tree = set_target(api, locref, ctx, m)
    run_batch(api, locref, ctx, tree, grid, None, poses, "shared", cap=0.02, shared=scan)


def test_nonfinite_points(api, locref, ctx):
    """NaN, +inf and −inf points inside a scan. P2P skips them (lists of −1, not counted as searched); under P2Plane they are searched
    — a NaN query goes to the tree, ±inf lies outside the grid — and get the lists of the product's own exact tree mode, which
    test_gpu_icp_hb.py holds against the oracle. The finite points get the oracle's lists in both."""
    c, rows = C.nonfinite_scan()
    grid, tree = set_target(api, locref, ctx, c["map"])
    scan, pose = c["scan"], c["pose"]
    fin = np.ones(len(scan), bool)
    fin[rows] = False
    with np.errstate(invalid="ignore"):
        q = q32_of(locref, scan, pose)
    b = ctx.batch([scan])
    try:
        ctx.search_stats_read(reset=True)
        for method, k in METHODS:
            hb_grid = ctx.icp_hb_batch(b, [pose], grid_opts(api, method))
            nn = ctx.debug_batch_nn(b, k)[0, :len(scan)].copy()
            st = ctx.search_stats_read(reset=True)
            print("nonfinite k=%d: searched %d walked %d" % (k, st["searched"], st["walked"]))
            check_lists(nn[fin], tree.knn(q[fin], k, approximate=False), "finite points k=%d" % k)
            hb_tree = ctx.icp_hb_batch(b, [pose], tree_opts(api, method))
            nn_tree = ctx.debug_batch_nn(b, k)[0, :len(scan)]
            ctx.search_stats_read(reset=True)
            if k == 1:
                assert np.all(nn[rows] == -1) and st["searched"] == len(scan) - len(rows)
            else:
                assert st["searched"] == len(scan) and st["walked"] >= len(rows)
            np.testing.assert_array_equal(nn[rows], nn_tree[rows])
            assert hb_grid.tobytes() == hb_tree.tobytes()
    finally:
        b.close()


def test_scans_that_finish_at_different_iterations(api, locref, ctx):
    """icp_align_batch in grid mode on four scans that converge after different numbers of iterations, one at once: both bin kernels
    drop a finished scan's queries (st[scan].done). Poses and stats have the bytes of the same batch under exact tree mode."""
    m, scans, inits = C.finishing_scans()
    set_target(api, locref, ctx, m)
    b = ctx.batch(scans)
    try:
        res = {}
        for name, opts in (("grid", grid_opts(api, api.P2PLANE, eps=C.FINISH_EPS)), ("tree", tree_opts(api, api.P2PLANE, eps=C.FINISH_EPS))):
            poses, st = ctx.icp_align_batch(b, inits, opts)
            res[name] = (poses, [(s["iterations"], s["converged"], s["status"], s["last_effective_num"], s["last_dx_norm"]) for s in st])
        iters = [s[0] for s in res["grid"][1]]
        print("finishing scans: iterations %s" % iters)
        assert len(set(iters)) == 4 and min(iters) == iters[3] <= 2
        assert all(s[1] == 1 and s[2] == 0 for s in res["grid"][1])
        assert res["grid"][0].tobytes() == res["tree"][0].tobytes() and res["grid"][1] == res["tree"][1]
    finally:
        b.close()
