"""Closed-form checks of tests/ndt_score_ref.py, the numpy restatement the GPU tests of the NDT fitness score compare against, and the
C ABI of the score on the host side: the four entry points exist and refuse NULL arguments."""
import ctypes

import numpy as np

import ndt_score_ref as ref


class _Identity:
    """Stand-in for the oracle's transform under the identity pose (the closed forms need no rotation)."""

    @staticmethod
    def transform_points(pose, pts):
        assert list(pose) == [0, 0, 0, 1, 0, 0, 0]
        return np.array(pts, dtype=np.float64)


IDENT = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def _sq(x):
    return x * x


def _one_voxel(key=(2, 3, 4), mu=(2.5, 3.25, 4.75), info=np.eye(3)):
    return ref.Table([key], [mu], [info])


def test_point_at_the_mean_scores_zero():
    t = _one_voxel()
    got = ref.score(_Identity, t, np.array([[2.5, 3.25, 4.75]], np.float32), IDENT)
    assert got == dict(score=0.0, inliers=1, finite_points=1)


def test_identity_information_gives_the_squared_distance():
    t = _one_voxel()
    pts = np.array([[2.0, 3.0, 4.0], [2.75, 3.5, 4.25], [2.5, 3.25, 4.0]], np.float32)
    res = ref.residuals(_Identity, t, pts, IDENT, n_nearby=1)
    e = pts.astype(np.float64) - [2.5, 3.25, 4.75]
    np.testing.assert_array_equal(res[:, 0], (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    got = ref.score(_Identity, t, pts, IDENT, n_nearby=1)
    assert got["inliers"] == 3 and got["score"] == res[:, 0].sum() / 3


def test_full_information_matrix_and_its_association():
    info = np.array([[2.0, 0.5, 0.0], [0.5, 3.0, 0.25], [0.0, 0.25, 1.0]])
    t = _one_voxel(info=info)
    p = np.array([[2.25, 3.5, 4.5]], np.float32)
    e = p[0].astype(np.float64) - [2.5, 3.25, 4.75]
    row = [(e[0] * info[0, c] + e[1] * info[1, c]) + e[2] * info[2, c] for c in range(3)]
    want = (row[0] * e[0] + row[1] * e[1]) + row[2] * e[2]
    assert ref.residuals(_Identity, t, p, IDENT, n_nearby=1)[0, 0] == want
    assert abs(want - e @ info @ e) < 1e-15


def test_gate_at_res_outlier_th():
    t = _one_voxel(key=(0, 0, 0), mu=(0.0, 0.0, 0.0))
    # ‖e‖² = 0.25 exactly: accepted at a threshold of 0.25 (res > th rejects), rejected just below it
    p = np.array([[0.5, 0.0, 0.0]], np.float32)
    assert ref.score(_Identity, t, p, IDENT, n_nearby=1, res_outlier_th=0.25) == dict(score=0.25, inliers=1, finite_points=1)
    assert ref.score(_Identity, t, p, IDENT, n_nearby=1, res_outlier_th=np.nextafter(0.25, 0)) == dict(score=float("inf"), inliers=0, finite_points=1)
    assert ref.gate_margin(ref.residuals(_Identity, t, p, IDENT, n_nearby=1), 0.25) == 0.0
    # a NaN residual (a voxel whose information is NaN) is never accepted
    tn = _one_voxel(key=(0, 0, 0), mu=(0.0, 0.0, 0.0), info=np.full((3, 3), np.nan))
    assert ref.score(_Identity, tn, p, IDENT, n_nearby=1)["inliers"] == 0


def test_minimum_over_two_voxels_and_probe_order_does_not_matter():
    # the point lies in voxel (1,0,0); its −x neighbour's mean is nearer than its own voxel's
    t = ref.Table([(1, 0, 0), (0, 0, 0)], [(1.9, 0.5, 0.5), (0.95, 0.5, 0.5)], [np.eye(3), np.eye(3)])
    p = np.array([[1.0625, 0.5, 0.5]], np.float32)
    res = ref.residuals(_Identity, t, p, IDENT)
    assert res.shape == (1, 7) and np.isnan(res[0, 2:]).all()
    assert res[0, 0] == _sq(1.0625 - 1.9) and res[0, 1] == _sq(1.0625 - 0.95)
    got = ref.score(_Identity, t, p, IDENT)
    assert got == dict(score=_sq(1.0625 - 0.95), inliers=1, finite_points=1)
    # CENTER sees only the point's own voxel
    assert ref.score(_Identity, t, p, IDENT, n_nearby=1)["score"] == _sq(1.0625 - 1.9)
    # the larger residual gated out, the smaller kept — and the other way round there is still one inlier
    assert ref.score(_Identity, t, p, IDENT, res_outlier_th=0.1)["score"] == _sq(1.0625 - 0.95)


def test_keys_truncate_toward_zero():
    q = np.array([[0.5, -0.5, -0.999], [-1.0, 1.0, -1.5], [0.999, -0.0, 2.5]])
    np.testing.assert_array_equal(ref.keys_of(q, 1.0), [[0, 0, 0], [-1, 1, -1], [0, 0, 2]])
    np.testing.assert_array_equal(ref.keys_of(q, 0.5), [[1, -1, -1], [-2, 2, -3], [1, 0, 5]])
    # (−1, 1) is ONE voxel per axis: a point at −0.5 finds voxel 0 with CENTER
    t = _one_voxel(key=(0, 0, 0), mu=(0.0, 0.0, 0.0))
    got = ref.score(_Identity, t, np.array([[-0.5, -0.5, 0.5]], np.float32), IDENT, n_nearby=1)
    assert got["inliers"] == 1 and got["score"] == 0.75
    # a key at the edge of the range is dropped, not wrapped
    far = np.array([[float(ref.BIAS), 0.0, 0.0]], np.float32)
    assert ref.score(_Identity, t, far, IDENT) == dict(score=float("inf"), inliers=0, finite_points=1)


def test_non_finite_points_are_not_counted_and_winner_rule():
    t = _one_voxel(key=(0, 0, 0), mu=(0.0, 0.0, 0.0))
    pts = np.array([[0.5, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0.25, 0, 0]], np.float32)
    got = ref.score(_Identity, t, pts, IDENT)
    assert got == dict(score=(0.25 + 0.0625) / 2, inliers=2, finite_points=2)
    fits = [dict(score=0.1, inliers=1, finite_points=10), dict(score=0.5, inliers=6, finite_points=10), dict(score=0.5, inliers=9, finite_points=10),
            dict(score=float("inf"), inliers=0, finite_points=10)]
    assert ref.winner(fits) == 1 and ref.winner(fits, 0.05) == 0 and ref.winner(fits, 0.95) == -1


def test_abi_exports_the_ndt_score_and_refuses_null_arguments(api):
    L = api.lib()
    for name in ("locgpu_ndt_fitness", "locgpu_ndt_fitness_batch", "locgpu_ndt_fitness_resident", "locgpu_ndt_init_search"):
        assert hasattr(L, name) and name in api.ABI_SYMBOLS, name
    invalid = -1  # LOCGPU_ERR_INVALID
    out = api.Fitness()
    pose = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    pts = np.zeros((4, 3), np.float32)
    best = ctypes.c_int(7)
    # no context at all: refused before anything is touched
    assert L.locgpu_ndt_fitness(None, pts.ctypes.data, 4, 12, pose.ctypes.data, 1, ctypes.byref(out)) == invalid
    assert L.locgpu_ndt_fitness_batch(None, None, pose.ctypes.data, ctypes.byref(out)) == invalid
    assert L.locgpu_ndt_fitness_resident(None, pose.ctypes.data, ctypes.byref(out)) == invalid
    assert L.locgpu_ndt_init_search(None, pts.ctypes.data, 4, 12, pose.ctypes.data, 1, None, pose.ctypes.data, ctypes.byref(out), None, ctypes.byref(best)) == invalid
    assert best.value == 7
