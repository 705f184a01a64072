"""The designed inputs of test_gpu_grid_lists.py reach the paths of the grid search they are named for — shown on the CPU with
grid_route_ref.ladder() in place of the library's grid (the GPU test repeats the routing on the dumped grid and holds the counters
of the library against it). Prints, per case and k, the share of every class of grid_route_ref.route()."""
import numpy as np
import pytest

import grid_list_cases as C
import grid_route_ref as R


def q32_of(locref, scan, pose):
    """What the kernels search for: float32 of the pose applied in double to the float32 scan."""
    return locref.transform_points(pose, np.ascontiguousarray(scan[:, :3], dtype=np.float64)).astype(np.float32)


@pytest.fixture(scope="module")
def routed(locref):
    out = {}
    for make in C.SINGLE:
        c = make()
        g = R.ladder(c["map"])
        q = q32_of(locref, c["scan"], c["pose"])
        cls = {k: R.route(g, q, k) for k in (5, 1)}
        for k in (5, 1):
            print("%-11s k=%d cell %.3f m dims %s tiles %d | %s" % (c["name"], k, g["cell"], "x".join(str(int(d)) for d in g["dims"]), g["n_tocc"], R.fmt(cls[k])))
        out[c["name"]] = (c, g, q, cls)
    return out


def _to_tree(cls):
    return int(np.sum((cls != "ring1") & (cls != "ring2")))


def test_ladder_targets_the_occupancy(routed):
    for name, (c, g, q, cls) in routed.items():
        assert g["n"] == len(c["map"]), name  # the designed maps hold no duplicate points
        assert g["n"] / g["n_occ"] >= R.TARGET_OCC and g["n"] / g["n_occ"] < R.TARGET_OCC * 1.3 ** 3 + 1, (name, g["n"] / g["n_occ"])


@pytest.mark.parametrize("name", [m.__name__ for m in C.SINGLE])
def test_the_share_the_tile_kernel_cannot_answer_is_under_the_cap(routed, name):
    c, g, q, cls = routed[name]
    assert np.abs(q.astype(np.float64) - c["want"])[np.isfinite(c["want"]).all(axis=1) & (np.abs(c["want"]) < 1e6).all(axis=1)].max() <= 0.02  # the scan lands where designed
    if c["cap"] is None:
        return
    for k in (5, 1):
        assert _to_tree(cls[k]) <= c["cap"] * len(q), (name, k, R.fmt(cls[k]))


def test_room_is_a_3d_neighbourhood_settled_by_ring_1(routed):
    c, g, q, cls = routed["room"]
    assert np.all(g["tdims"] >= 2) and g["n_tocc"] >= 50
    assert np.mean(cls[5] == "ring1") >= 0.95 and np.mean(cls[1] == "ring1") >= 0.95
    blocks = [len(R.block_leaves(g, int(t))) for t in g["tile_lin"]]
    assert max(blocks) <= R.STAGE_CAP
    print("room: largest block %d leaves" % max(blocks))


def test_sheet_and_line_have_axes_of_one_cell(routed):
    assert routed["sheet"][1]["dims"][2] == 1 and np.all(routed["sheet"][1]["dims"][:2] > 8)
    assert list(routed["line"][1]["dims"][1:]) == [1, 1] and routed["line"][1]["dims"][0] > 256
    for name in ("sheet", "line"):
        for k in (5, 1):
            assert np.mean(routed[name][3][k] == "ring1") >= 0.9


def test_wide_fills_the_bin_kernels_hash(routed):
    c, g, q, cls = routed["wide"]
    _, _, lin = R.query_cells(g, q)
    assert g["n_tocc"] >= 300 and len(q) == 2048
    per_block = [len(np.unique(lin[i:i + R.RANGE_Q][lin[i:i + R.RANGE_Q] >= 0])) for i in range(0, len(q), R.RANGE_Q)]
    print("wide: distinct tile keys per 256-query block: %s" % per_block)
    assert min(per_block) >= 200


def hot_runs(g, q, hot):
    """[(start, length)] of the hot tiles' runs in the tile-sorted query list (records are in tile_lin order)."""
    _, _, lin = R.query_cells(g, q)
    lin = lin[np.isin(lin, g["tile_lin"])]
    tiles, counts = np.unique(lin, return_counts=True)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return [(int(start[tiles == t][0]), int(counts[tiles == t][0])) for t in hot]


def test_hot_tiles_runs_cross_range_boundaries(routed):
    c, g, q, cls = routed["hot_tiles"]
    runs = hot_runs(g, q, c["hot"])
    print("hot tiles: (start, length) of the runs after the sort by tile: %s" % runs)
    for (s, n), want in zip(runs, C.HOT_RUNS):
        assert n >= want  # the run, plus what the spread queries add to the tile
    crossed = [(s + n - 1) // R.RANGE_Q - s // R.RANGE_Q for s, n in runs]
    inside = [s % R.RANGE_Q != 0 for s, n in runs]
    assert any(x == 1 and i for x, i in zip(crossed, inside)) and any(x >= 2 and i for x, i in zip(crossed, inside)), (runs, crossed)


def test_sparse_half_needs_the_shell(routed):
    c, g, q, cls = routed["sparse_half"]
    assert np.mean(cls[5] == "ring2") >= c["ring2_share"]
    assert np.mean(cls[1] == "ring1") >= 0.9


def clump_neighbours(g, q, cls):
    """Queries the tile kernel answers in a tile that touches a tile whose block is refused."""
    _, _, lin = R.query_cells(g, q)
    td = g["tdims"]
    txyz = lambda t: np.stack([t % td[0], (t // td[0]) % td[1], t // (td[0] * td[1])], -1)
    refused = txyz(np.unique(lin[cls == "no_fit"]))
    mine = txyz(lin)
    near = (np.abs(mine[:, None, :] - refused[None, :, :]).max(axis=2) <= 1).any(axis=1)
    return int(np.sum(near & ((cls == "ring1") | (cls == "ring2"))))


def test_clump_refuses_some_blocks_and_stages_their_neighbours(routed):
    c, g, q, cls = routed["clump"]
    for k in (5, 1):
        assert np.mean(cls[k] == "no_fit") >= c["no_fit_share"]
        assert clump_neighbours(g, q, cls[k]) >= 20
    assert max(np.bincount(np.searchsorted(g["tile_lin"], g["leaf_tile"]))) <= 65535


def test_offset_slack_comes_from_max_abs(routed):
    c, g, q, cls = routed["offset"]
    assert g["slack"] > 50 * 1e-3 * g["cell"] and g["slack"] < 0.5 * g["cell"]
    assert g["dims"][2] == 1


def test_ties_reach_the_tile_kernel(routed):
    """The 16³ lattice is a filled volume: the blocks of its interior tiles exceed the stage, so most of its queries are no_fit, ties
    or not, and the tile kernel meets the ties of the outer tiles only. Every block of the flat lattice fits: all its tied queries are
    the tile kernel's to detect."""
    c, g, q, cls = routed["ties"]
    for k in (5, 1):
        assert np.sum(cls[k] == "tie") >= 300 and np.sum(cls[k] == "no_fit") >= 300
    c, g, q, cls = routed["ties_flat"]
    for k in (5, 1):
        assert np.sum(cls[k] == "tie") >= 1100 and np.sum(cls[k] == "no_fit") == 0
        assert np.sum(np.isin(cls[k], ["ring1", "ring2"])) >= 400  # the noisy ones are answered


def test_room_edges_leave_the_grid(routed):
    c, g, q, cls = routed["room_edges"]
    for k in (5, 1):
        assert np.sum(cls[k] == "outside") >= c["n_outside_min"]
        assert cls[k][-102] != "outside" and cls[k][-101] != "outside"  # the two corners of the bounding box are inside


def test_tiny_targets_have_axes_of_one_to_three_cells():
    for name, m, q in C.tiny_targets():
        g = R.ladder(m)
        cls = R.route(g, q, 5)
        print("%-9s dims %s | %s" % (name, list(g["dims"]), R.fmt(cls)))
        assert np.all(g["dims"] <= 8)
        if g["n"] < 5:
            assert not np.any(np.isin(cls, ["ring1", "ring2", "tie"]))  # fewer than K leaves: never the tile kernel's answer
        if name == "row12":
            assert list(g["dims"]) == [3, 1, 1] and np.sum(np.isin(cls, ["ring1", "ring2"])) >= 60


def test_batches_on_the_room_map_stay_under_the_cap(locref):
    m, scans, poses = C.ragged_batch()
    g = R.ladder(m)
    m2, shared, poses2 = C.shared_pair()
    for what, ss, pp in (("ragged", scans, poses), ("shared", [shared, shared], poses2)):
        for k in (5, 1):
            cls = np.concatenate([R.route(g, q32_of(locref, s, p), k) for s, p in zip(ss, pp) if len(s)])
            print("%-7s k=%d | %s" % (what, k, R.fmt(cls)))
            assert _to_tree(cls) <= 0.02 * len(cls)


def test_finishing_scans_take_different_numbers_of_iterations(locref):
    m, scans, inits = C.finishing_scans()
    icp = locref.Icp(method=locref.P2PLANE, use_ann=False, eps=C.FINISH_EPS)
    icp.set_target(m)
    iters = [icp.align(s, p)["iters"] for s, p in zip(scans, inits)]
    print("finishing scans: the oracle's iterations %s" % iters)
    assert len(set(iters)) == 4 and min(iters) == iters[3] <= 2
