"""The inputs of tests/test_gpu_fitness_points.py are what they claim (tests/fitness_cases.py), checked without a device: the exact
world is exact, its gate points sit on the gate, a float32 squares to the non-dyadic gate, the per-point NDT inputs make the minimum
over the probed voxels matter, and the recorded unit of the NDT restatement is not below what is measured here."""
import numpy as np
import pytest

import fitness_cases as cases
import ndt_score_ref



@pytest.fixture(scope="module")
def world():
    return cases.exact_world()


@pytest.fixture(scope="module")
def oracle_table(locref, small_world):
    ndt = locref.Ndt()
    ndt.set_target(small_world["map"])
    return ndt_score_ref.Table(*ndt.dump())


def _se3_apply(pose, v):
    """se3_apply of csrc/device_math.hpp (and the oracle's transform) restated in numpy FP64, operation by operation."""
    q, t = pose[:4], pose[4:]
    qv = np.broadcast_to(q[:3], v.shape)
    uv = np.cross(qv, v)
    uv = uv + uv
    return ((v + q[3] * uv) + np.cross(qv, uv)) + t[None, :]


def test_the_three_poses_are_exact(locref, world):
    """Integer arithmetic = the oracle's FP64 transform = se3_apply's formula = the float32 cast of either, on all 131 073 points."""
    src = world["src"]
    assert src.dtype == np.float32 and len(src) == 131073 and np.array_equal(src.astype(np.float64) * cases.Q, world["src_int"])
    for pose in world["poses"]:
        want = cases.exact_apply(pose, world["src_int"]) / float(cases.Q)
        got = locref.transform_points(pose[0], src.astype(np.float64))
        assert np.array_equal(got, want) and np.array_equal(_se3_apply(pose[0], src.astype(np.float64)), want)
        assert np.array_equal(got.astype(np.float32).astype(np.float64), want)
        # at most 2.5 m outside the slab
        assert np.abs(want[:, :2]).max() <= 18.5 and np.abs(want[:, 2]).max() <= 3.0
    assert [tuple(p[1]) for p in world["poses"]] == [(1, 1, 1), (-1, -1, 1), (1, -1, -1)]  # a half-turn exercises the rotation terms
    print("exact poses: integer arithmetic, the oracle's transform and se3_apply's formula agree, bit-equal, %d points x 3 poses" % len(src))


def test_the_integer_distance_is_the_minimum_over_all_map_points(world):
    """exact_d2 (per axis, product grid) against the minimum over all 12 675 (3 267) map points in integers, and against the float32
    brute force the per-point ICP test uses, on a sample; every d² is below 2^5."""
    assert len(world["map"]) == 12675 and len(world["edge_map"]) == 3267
    pick = np.r_[world["at_gate"][:40], world["above_gate"][:40], np.arange(0, 131073, 331)]
    for pose in world["poses"]:
        w = cases.exact_apply(pose, world["src_int"])
        for grid, m in ((world["grid"], world["map"]), (world["edge_grid"], world["edge_map"])):
            d2 = cases.exact_d2(grid, w)
            assert d2.max() < 32 * cases.Q2
            assert np.array_equal(d2[pick], cases.exact_d2_brute(m, w[pick]))
            f = cases.brute_d2((w[pick] / float(cases.Q)).astype(np.float32), m)
            assert np.array_equal(f.astype(np.float64) * cases.Q2, d2[pick])
    print("exact_d2: bit-equal, %d points x 3 poses x 2 maps" % len(pick))


def test_the_host_tree_of_the_lattice_is_within_the_depth_limit(api, world):
    depths = [cases.host_tree_depth(api, world["map"]), cases.host_tree_depth(api, world["edge_map"])]
    print("host tree depth of the lattice %d, of the edge lattice %d (limit 64)" % tuple(depths))
    assert max(depths) <= 64


def test_points_on_the_gate_and_one_step_above(world):
    w = cases.exact_apply(world["poses"][1], world["src_int"])
    d2 = cases.exact_d2(world["grid"], w)
    at, above = d2 == cases.Q2, d2 == cases.Q2 + 1
    print("d2 == 1.0: %d points, d2 == 1.0 + 2^-8: %d points (want >= 100 of each)" % (at.sum(), above.sum()))
    assert at.sum() >= 100 and above.sum() >= 100
    assert at[world["at_gate"]].all() and above[world["above_gate"]].all() and len(world["at_gate"]) == len(world["above_gate"]) == 128
    assert world["at_gate"].max() < 4096 and world["above_gate"].max() < 4096
    assert cases.gate_int(1.0) == cases.Q2 and cases.gate_int(float("inf")) is None
    # every length and every gate has inliers and refused points (but the one-point scan)
    for rng in (0.3, 1.0):
        for n in cases.ROW_LENGTHS[1:]:
            f, _ = cases.exact_fitness(d2[:n], rng)
            assert 0 < f["inliers"] < n
    assert [(n + 1023) // 1024 for n in cases.ROW_LENGTHS] == [1, 1, 1, 1, 1, 1, 2, 4, 64, 65, 129]


def test_a_float_squares_to_the_gate_that_is_not_dyadic():
    gate = cases.gate_of(0.3)
    assert gate == np.float32(0.3 * 0.3) and float(gate) * 2 ** 8 % 1 != 0  # the double product cast once, and no multiple of 2^-8
    found = cases.gate_neighbours(0.3)
    assert found is not None
    dx_at, dx_above = found
    assert dx_at.dtype == dx_above.dtype == np.float32 and dx_above == np.nextafter(dx_at, np.float32(np.inf))
    assert np.float32(dx_at * dx_at) == gate and np.float32(dx_above * dx_above) > gate
    m, at, above = cases.gate_world(dx_at, dx_above)
    assert np.array_equal(cases.brute_d2(at, m), np.full(16, gate)) and (cases.brute_d2(above, m) > gate).all()
    print("max_range 0.3: gate %.9g = fl32(%.9g^2) < fl32(%.9g^2)" % (gate, dx_at, dx_above))


def test_icp_point_inputs_straddle_every_gate(locref, small_world):
    inp = cases.icp_point_inputs(small_world)
    assert len(inp["map"]) == 20000 and len(inp["scan"]) == 2000 + 64 + 400
    fin = np.isfinite(inp["scan"]).all(axis=1)
    assert (~fin).sum() == 7 and fin[:2064].all()
    for name, pose in inp["poses"].items():
        f, d2 = cases.icp_point_ref(locref, inp, pose)
        assert np.array_equal(f, fin) and np.isnan(d2[~fin]).all() and not np.isnan(d2[fin]).any()
        far = d2[2000:2064]
        assert far.min() > 30.0 ** 2 * 0.9 and far.max() < 1100.0 ** 2
        for rng in (0.3, 1.0):
            inl = d2[fin] <= cases.gate_of(rng)
            print("%s, max_range %.1f: %d inliers, %d refused" % (name, rng, inl.sum(), (~inl).sum()))
            assert inl.sum() >= 100 and (~inl).sum() >= 100
        assert np.isinf(d2[2064 + 200]) and np.isinf(d2[2064 + 201])  # the 1e30 rows: finite points whose d² overflows float32


@pytest.fixture(scope="module")
def ndt_inputs(locref, small_world, oracle_table):
    return cases.ndt_point_inputs(locref, oracle_table, small_world)


def test_ndt_inputs_make_the_minimum_matter(locref, ndt_inputs, oracle_table):
    """Decided from the 60-digit restatement alone: nothing excluded, and the counts the per-point test leans on."""
    not_centre = rescued = none = pairs = 0
    for name, pose, pts in ndt_inputs:
        for n_nearby in (7, 1):
            r = cases.ndt_point_ref(oracle_table, pts, pose, n_nearby)
            pairs += r["pairs"]
            assert r["key_margin"].min() > cases.KEY_MARGIN and r["gate_margin"].min() > cases.GATE_REL
            _, which, nc, rs, no = cases.classify(r["res"])
            assert np.array_equal(which, r["which"]) and np.array_equal(no, ~r["inlier"])
            not_centre, rescued, none = not_centre + nc.sum(), rescued + rs.sum(), none + no.sum()
            print("%s, %d voxels probed: %d points, smallest not the centre's %d, centre refused or absent and a neighbour accepted %d, no accepted voxel %d; "
                  "nearest key margin %.2e, nearest gate margin %.2e" % (name, n_nearby, len(pts), nc.sum(), rs.sum(), no.sum(), r["key_margin"].min(), r["gate_margin"].min()))
    print("in all: %d / %d / %d (want >= 50 / 20 / 20), %d point-voxel pairs at 60 digits" % (not_centre, rescued, none, pairs))
    assert not_centre >= 50 and rescued >= 20 and none >= 20
    assert pairs <= 4000


def test_unit_of_the_ndt_restatement(locref, ndt_inputs, oracle_table):
    """The numpy restatement (ndt_score_ref.residuals_at on the oracle's transform) against the 60-digit value in err / (u·S): the unit
    recorded in fitness_cases.UNIT is not below it, and never below 1."""
    worst = 0.0
    for name, pose, pts in ndt_inputs:
        r = cases.ndt_point_ref(oracle_table, pts, pose, 7)
        got = ndt_score_ref.residuals(locref, oracle_table, pts, pose, cases.VOXEL, 7)
        assert np.array_equal(np.isnan(got), np.isnan(r["res"]))
        for i, j in zip(*np.nonzero(~np.isnan(got))):
            worst = max(worst, cases.err_in_units(got[i, j], r["res_mp"][i][j], r["S"][i, j]))
    print("numpy restatement against 60 digits: worst err / (u S) %.3g; recorded unit %.3g, bar %.3g" % (worst, cases.UNIT, cases.BAR_FACTOR * cases.UNIT))
    assert worst <= cases.UNIT and cases.UNIT >= 1.0


def test_ndt_gate_cases_put_the_residual_on_the_threshold(oracle_table):
    """The restatement's residual of every gate case is the threshold, bit for bit, in the centre voxel."""
    gate = cases.ndt_gate_cases(oracle_table)
    assert len(gate) == 8
    for t, th, key in gate:
        v = oracle_table.find(ndt_score_ref.keys_of(t[None, :], cases.VOXEL))[0]
        assert v >= 0 and oracle_table.packed[v] == key
        res = ndt_score_ref.residuals_at(oracle_table, t[None, :], cases.VOXEL, 1)[0, 0]
        assert res == th and 0 < th < 1e6
        both = ndt_score_ref.score_from_residuals(np.array([[res]]), th, 1), ndt_score_ref.score_from_residuals(np.array([[res]]), np.nextafter(th, 0.0), 1)
        assert both[0]["inliers"] == 1 and both[1]["inliers"] == 0
    print("NDT gate cases: residual == threshold, bit-equal, %d voxels; thresholds %s" % (len(gate), ["%.6g" % th for _, th, _ in gate]))
