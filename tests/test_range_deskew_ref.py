"""The numpy restatement of the motion-compensated range-image ingest (tests/range_deskew_ref.py) checked without a GPU: its matrices
undo a rigid world's apparent motion (the definition's sense and direction), its interval rule is math::PoseInterp's
(math_utils.h:470-517), and the error of its float64 arithmetic against the same code in longdouble — the unit
tests/test_gpu_range_deskew.py measures the device in — is measured and printed."""
import numpy as np
import pytest

import range_deskew_cases as cases
import range_deskew_ref as ref


@pytest.mark.parametrize("name", cases.TRACKS)
def test_matrices_undo_the_motion_of_a_rigid_world(name):
    """World points W seen from the moving sensor at a column's time, p_c = T(t_c)^-1 W, must land on T(t_ref)^-1 W, to 1e-9 m."""
    times, poses = cases.track(name)
    rng = np.random.default_rng(5)
    n_cols = 157
    W = cases.T0 + rng.uniform(-50.0, 50.0, (n_cols, 3))
    worst = 0.0
    for table in cases.COL_TABLES:
        col = cases.col_times(times, n_cols, table)
        for which in cases.REF_TIMES:
            r = cases.ref_time(times, col, which)
            assert not ref.refused(times, col, r)
            pc, pr = ref.pose_at(times, poses, col), ref.pose_at(times, poses, [r])[0]
            Rc, Rr = ref.quat_to_R(pc[:, :4]), ref.quat_to_R(pr[:4])
            seen = np.einsum("nji,nj->ni", Rc, W - pc[:, 4:])  # R_c^T (W - t_c)
            want = (W - pr[4:]) @ Rr                           # R_r^T (W - t_r)
            M = ref.matrices(times, poses, col, r)
            got = np.einsum("nij,nj->ni", M[:, :, :3], seen) + M[:, :, 3]
            worst = max(worst, float(np.abs(got - want).max()))
    print("%s: worst |M p_c - T(t_ref)^-1 W| = %.2e m (bar 1e-9)" % (name, worst))
    assert worst <= 1e-9


def test_pose_at_follows_pose_interp():
    """The interval and the three shortcuts of math_utils.h:470-517, restated by a plain loop over the knots."""
    for name in cases.TRACKS:
        times, poses = cases.track(name)
        K = len(times)
        qs = np.concatenate([times, 0.5 * (times[1:] + times[:-1]), [times[-1] + 0.2, np.nextafter(times[1], 0.0), np.nextafter(times[1], 1.0)]])
        got = ref.pose_at(times, poses, qs)
        for q, g in zip(qs, got):
            if q > times[-1]:
                assert np.array_equal(g, poses[-1])
                continue
            j = 0
            for i in range(K - 1):  # :489-497
                if times[i] < q <= times[i + 1]:
                    j = i
                    break
            dt = times[j + 1] - times[j]
            if abs(dt) < 1e-6:
                assert np.array_equal(g, poses[j]), (name, q)
                continue
            s = (q - times[j]) / dt
            assert np.array_equal(g[4:], poses[j, 4:] * (1 - s) + poses[j + 1, 4:] * s), (name, q)
            if s == 0.0 or s == 1.0:  # a knot's own time gives the knot's rotation (up to the quaternion's sign)
                k = poses[j] if s == 0.0 else poses[j + 1]
                assert abs(abs(g[:4] @ k[:4]) - 1.0) < 1e-14
            assert abs(np.linalg.norm(g[:4]) - 1.0) < 1e-12
    # the negated knot: the interpolated rotation still lies between its neighbours
    times, poses = cases.track("k9_neg")
    mid = ref.pose_at(times, poses, [0.5 * (times[3] + times[4]), 0.5 * (times[4] + times[5])])
    assert abs(mid[0, :4] @ poses[3, :4]) > 0.9999 and abs(mid[1, :4] @ poses[5, :4]) > 0.9999


def test_time_refusals_of_the_restatement():
    times, _ = cases.track("k9_neg")
    col = cases.col_times(times, 64, "uniform")
    assert not ref.refused(times, col, times[-1] + 0.5)
    assert ref.refused(times, col, times[-1] + 0.6) and ref.refused(times, col, times[0] - 1e-9)
    early = col.copy()
    early[7] = times[0] - 1e-6
    assert ref.refused(times, early, col[-1])


def test_apply_is_the_double_matrix_transform():
    rng = np.random.default_rng(2)
    pts = np.zeros((50, 4), np.float32)
    pts[:, :3] = rng.uniform(-80, 80, (50, 3))
    eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (4, 1, 1))
    cols = rng.integers(0, 4, 50)
    assert ref.apply(pts, cols, eye).tobytes() == pts.tobytes()
    shift = eye.copy()
    shift[2, :, 3] = (1.0, -2.0, 0.5)
    out = ref.apply(pts, cols, shift)
    moved = cols == 2
    assert np.array_equal(out[~moved], pts[~moved]) and np.array_equal(out[moved, :3], (pts[moved, :3].astype(np.float64) + (1.0, -2.0, 0.5)).astype(np.float32))
    assert not out[:, 3].any()


def test_unit_of_the_float64_restatement():
    """The unit of tests/test_gpu_range_deskew.py per track: float64 against longdouble, in multiples of eps * max(1, max ||t||)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "numpy.longdouble is no wider than float64 here: the unit cannot be measured"
    for name in cases.TRACKS:
        _, poses = cases.track(name)
        for n_cols in (300, 1231):
            u = cases.unit(name, n_cols)
            print("%-10s n_cols %4d: unit %.3f x eps * max(1, max||t||) = %.3e" % (name, n_cols, u, u * cases.scale(poses)))
            # the arithmetic is a few dozen float64 operations on values of magnitude <= max(1, ||t||): a unit far from one would mean
            # that the restatement, not rounding, is what differs
            assert 0.0 < u < 16.0, (name, u)
