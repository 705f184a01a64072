"""The tracks, column-time tables and reference times the deskewed range-image ingest is tested on, shared by test_range_deskew_ref.py
(no GPU) and test_gpu_range_deskew.py, and the unit the device's matrices are measured in.

Tracks: translations near (100, -40, 2) m, so that the cancellation in t_c - t_r is exercised; knots over a 0.1 s sweep.
  k2        K = 2: 20 degrees about a skew axis and 2 m
  k9_neg    K = 9, 3 degrees and 0.2 m per knot, knot 4's quaternion negated (slerp's d < 0 branch on both sides of it)
  k33_small K = 33, 1e-4 rad per knot (acos next to 1)
  k5_equalq K = 5, one quaternion for every knot and a moving translation (slerp's ad >= 1 - eps branch)
  k4_short  K = 4 with the interval [0.05, 0.05 + 5e-7] (PoseInterp's |dt| < 1e-6 rule)
  k256      K = 256, the largest
Column times of a sensor with n_cols columns: uniform over the knot span; the same rolled by a third (not increasing: a sensor that
starts mid-turn); entries exactly on knot times, the first and last knot included; entries 0.2 s behind the last knot.
Reference times: the last column's, the first knot's, one mid-sweep."""
import numpy as np

import range_deskew_ref as ref

EPS = 2.0 ** -52
BAR_FACTOR = 8  # the rule of tests/test_gpu_ndt_hb.py: 8 units
T0 = np.array([100.0, -40.0, 2.0])
SPAN = 0.1
TRACKS = ("k2", "k9_neg", "k33_small", "k5_equalq", "k4_short", "k256")
COL_TABLES = ("uniform", "rolled", "on_knots", "late")
REF_TIMES = ("last_col", "first_knot", "mid")


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.append(a * np.sin(0.5 * angle), np.cos(0.5 * angle))


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz])
    return q / np.linalg.norm(q)


Q0 = _quat((0.2, -0.3, 0.9), 0.7)


def _chain(K, axis, step, velocity, wobble=0.0):
    """K knots over SPAN: a rotation of `step` rad per knot about `axis` (tilted by `wobble` from knot to knot), translation T0 + velocity * t."""
    times = np.linspace(0.0, SPAN, K)
    poses = np.zeros((K, 7))
    q = Q0
    for k in range(K):
        if k:
            q = _qmul(q, _quat(np.asarray(axis) + wobble * np.array([np.sin(k), np.cos(2 * k), 0.0]), step))
        poses[k, :4] = q
        poses[k, 4:] = T0 + np.asarray(velocity) * times[k]
    return times, poses


def track(name):
    """(knot_times [K], knot_poses [K, 7]) float64."""
    if name == "k2":
        times, poses = _chain(2, (1.0, 2.0, 3.0), np.deg2rad(20.0), (12.0, -15.0, 5.5))  # 2.0 m over the sweep
    elif name == "k9_neg":
        times, poses = _chain(9, (0.3, -0.2, 1.0), np.deg2rad(3.0), (13.0, 9.0, -1.0))
        poses[4, :4] = -poses[4, :4]
    elif name == "k33_small":
        times, poses = _chain(33, (0.1, 0.2, 1.0), 1e-4, (15.0, 1.0, 0.2))
    elif name == "k5_equalq":
        times, poses = _chain(5, (0.0, 0.0, 1.0), 0.0, (-14.0, 6.0, 0.5))
        poses[:, :4] = Q0
    elif name == "k4_short":
        times, poses = _chain(4, (0.5, 0.1, 1.0), np.deg2rad(2.0), (10.0, -12.0, 1.0))
        times = np.array([0.0, 0.05, 0.05 + 5e-7, SPAN])
        poses[:, 4:] = T0 + np.array([10.0, -12.0, 1.0]) * times[:, None]
    elif name == "k256":
        times, poses = _chain(256, (0.2, 0.1, 1.0), np.deg2rad(0.1), (15.0, -3.0, 0.4), wobble=0.3)
    else:
        raise KeyError(name)
    return times, poses


def col_times(times, n_cols, table):
    K, first, last = len(times), times[0], times[-1]
    col = np.linspace(first, last, n_cols)
    if table == "rolled":
        col = np.roll(col, n_cols // 3)
    elif table == "on_knots":
        at = np.unique(np.linspace(0, n_cols - 1, min(K, n_cols)).astype(int))
        col[at] = times[np.linspace(0, K - 1, len(at)).astype(int)]  # knot 0 and knot K - 1 among them
        assert col[0] == first and col[-1] == last
    elif table == "late":
        col[-max(n_cols // 10, 1):] = last + 0.2
        col[min(3, n_cols - 1)] = last + 0.2
    elif table != "uniform":
        raise KeyError(table)
    return col


def ref_time(times, col, which):
    return {"last_col": col[-1], "first_knot": times[0], "mid": times[0] + 0.537 * (times[-1] - times[0])}[which]


def scale(poses):
    """eps * max(1, max ||t||): what one unit of a track is a multiple of."""
    return EPS * max(1.0, float(np.linalg.norm(np.asarray(poses)[:, 4:], axis=1).max()))


def unit(name, n_cols=300):
    """The largest deviation of the float64 restatement's matrices from the longdouble restatement's over every column table and
    reference time of track `name`, in multiples of scale(): the error of the defined float64 arithmetic itself, which the device
    repeats operation for operation except for acos and sin."""
    times, poses = track(name)
    worst = 0.0
    for table in COL_TABLES:
        col = col_times(times, n_cols, table)
        for which in REF_TIMES:
            r = ref_time(times, col, which)
            m64 = ref.matrices(times, poses, col, r, np.float64)
            m80 = ref.matrices(times, poses, col, r, np.longdouble)
            worst = max(worst, float(np.abs(m64.astype(np.longdouble) - m80).max()))
    return worst / scale(poses)
