"""locgpu_motion_from_poses restated in numpy float64, line by line from include/locgpu.h ("Deskew of a resident batch", the comment of
locgpu_motion_from_poses): one IEEE double operation per written operation, in the header's order, nothing normalised. Test
infrastructure: what the host helper is held to, byte for byte.

A pose is 7 float64: quaternion x, y, z, w, then translation."""
import numpy as np

F = np.float64


def quat_to_R(q):
    """Eigen's toRotationMatrix in the header's order."""
    x, y, z, w = (F(v) for v in q)
    tx, ty, tz = F(2.0) * x, F(2.0) * y, F(2.0) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = F(1.0)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], F)


def quat_mul(a, b):
    """a (x) b."""
    ax, ay, az, aw = (F(v) for v in a)
    bx, by, bz, bw = (F(v) for v in b)
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by + ay * bw) + az * bx) - ax * bz
    z = ((aw * bz + az * bw) + ax * by) - ay * bx
    return np.array([x, y, z, w], F)


def rotate(q, v):
    """R(q) v, each row (R[r][0] v0 + R[r][1] v1) + R[r][2] v2."""
    R = quat_to_R(q)
    v = [F(c) for c in v]
    return np.array([(R[r, 0] * v[0] + R[r, 1] * v[1]) + R[r, 2] * v[2] for r in range(3)], F)


def inverse(p):
    """inv(q, t) = (c, -(R(c) t)) with c = (-x, -y, -z, w)."""
    p = np.asarray(p, F)
    c = np.array([-p[0], -p[1], -p[2], p[3]], F)
    return np.concatenate([c, -rotate(c, p[4:])])


def compose(a, b):
    """(q1, t1) * (q2, t2) = (q1 (x) q2, t1 + R(q1) t2)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    rt = rotate(a[:4], b[4:])
    return np.concatenate([quat_mul(a[:4], b[:4]), np.array([a[4 + r] + rt[r] for r in range(3)], F)])


def extrapolate(a, b):
    """(T_a * inv(T_b)) * T_a: the reference's predict_pos = result_pos * last_pose.inverse() * result_pos (loc.cpp:232)."""
    return compose(compose(a, inverse(b)), a)


def motion_from_poses(poses, stamps):
    """(knot_times [n, 3], knot_poses [n, 3, 7]): scan i gets the poses and stamps of scans i-1, i, i+1; before the first scan
    (T[0] * inv(T[1])) * T[0] at 2.0 * t[0] - t[1], after the last (T[n-1] * inv(T[n-2])) * T[n-1] at 2.0 * t[n-1] - t[n-2]."""
    poses, t = np.asarray(poses, F).reshape(-1, 7), np.asarray(stamps, F).reshape(-1)
    n = len(t)
    before, after = extrapolate(poses[0], poses[1]), extrapolate(poses[n - 1], poses[n - 2])
    t_before, t_after = F(2.0) * t[0] - t[1], F(2.0) * t[n - 1] - t[n - 2]
    kt, kp = np.zeros((n, 3), F), np.zeros((n, 3, 7), F)
    for i in range(n):
        for k in range(3):
            j = i - 1 + k
            kt[i, k] = t_before if j < 0 else t_after if j >= n else t[j]
            kp[i, k] = before if j < 0 else after if j >= n else poses[j]
    return kt, kp
