"""Known answers of tests/loam_score_ref.py, the CPU statement of the LOAM matcher's joint score: worked out by hand, no library."""
import numpy as np

import loam_score_ref as ref

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def test_two_point_maps_pool_the_inliers_of_both_classes():
    surf_map = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    edge_map = np.array([[0, 5, 0], [0, -5, 0]], np.float32)
    # under a shift of +1 m in x: surface d² = 1 (-2 → -1, 1 m from the origin), 4 (11 → 12, 2 m from 10), 16 (5 → 6: beyond the 3 m range)
    surf = np.array([[-2, 0, 0], [11, 0, 0], [5, 0, 0]], np.float32)
    edge = np.array([[-1, 5.5, 0], [np.nan, 0, 0]], np.float32)  # d² = 0.25; the NaN point is no query
    pose = np.array([0, 0, 0, 1, 1.0, 0, 0])
    joint, s, e = ref.joint_score(edge_map, surf_map, edge, surf, pose, max_range=3.0)
    assert (s["inliers"], s["finite_points"], s["score"]) == (2, 3, 2.5)
    assert (e["inliers"], e["finite_points"], e["score"]) == (1, 1, 0.25)
    # the pooled mean (1 + 4 + 0.25) / 3 — not the sum of the two means, 2.75
    assert (joint["inliers"], joint["finite_points"], joint["score"]) == (3, 4, 1.75)
    # a quarter turn about z: (1, 0, 0) → (0, 1, 0), 4 m from the edge map's (0, 5, 0)
    turn = np.array([0, 0, np.sin(np.pi / 4), np.cos(np.pi / 4), 0, 0, 0])
    _, _, e2 = ref.joint_score(edge_map, surf_map, np.array([[1, 0, 0]], np.float32), None, turn, max_range=5.0)
    assert e2["inliers"] == 1 and abs(e2["score"] - 16.0) < 1e-5


def test_a_class_switched_off_adds_nothing():
    surf_map = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    surf = np.array([[0.5, 0, 0], [9, 0, 0]], np.float32)
    joint, s, e = ref.joint_score(None, surf_map, None, surf, IDENTITY, max_range=2.0)
    assert e == dict(score=float("inf"), inliers=0, finite_points=0)
    assert joint == s == dict(score=0.625, inliers=2, finite_points=2)


def test_no_inlier_in_either_class_is_infinity_and_never_wins():
    maps = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    far = np.array([[50, 50, 0]], np.float32)
    joint, s, e = ref.joint_score(maps, maps, far, far, IDENTITY, max_range=1.0)
    assert joint == dict(score=float("inf"), inliers=0, finite_points=2) and s["score"] == e["score"] == float("inf")
    near = ref.joint_score(maps, maps, np.array([[0.5, 0, 0]], np.float32), maps[:1], IDENTITY, max_range=1.0)[0]
    assert (near["inliers"], near["score"]) == (2, 0.125)
    assert ref.winner([joint, near, near]) == 1  # the tie goes to the lower index, the candidate without inliers never qualifies
    assert ref.winner([joint]) == -1 and ref.winner([near], min_inlier_ratio=1.1) == -1


def test_the_slab_search_is_the_all_pairs_search():
    """nn_d2 skips map points that cannot be the nearest; what it returns is what evaluating every pair returns, bit for bit."""
    rng = np.random.default_rng(5)
    m = (rng.random((20000, 3)) * [80, 80, 6] - [40, 40, 1]).astype(np.float32)
    q = (rng.random((600, 3)) * [90, 90, 8] - [45, 45, 2]).astype(np.float32)  # some queries lie outside the map's box
    q[:5] = m[:5]  # and some on a map point
    got, want = ref.nn_d2(m, q), ref.nn_d2(m, q, all_pairs=True)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[:5] == 0).all()
