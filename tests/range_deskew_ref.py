"""Motion compensation at decode restated in numpy (include/locgpu.h, "Range-image ingest, motion-compensated"):
math::PoseInterp's rule (LocUtils/include/LocUtils/common/math_utils.h:470-517) with Eigen's slerp, the matrix of a column and its
application to CloudConver::Conver's survivors (LocUtils/src/subscriber/cloud_subscriber.cpp:7-29). Test infrastructure: what
locgpu_batch_upload_ranges_deskew and locgpu_cloud_upload_ranges_deskew are held to.

Every function takes ``dtype``: numpy.float64 restates the device arithmetic operation for operation (numpy fuses nothing; only
arccos and sin may round differently from the device library's), numpy.longdouble is the same code with every operation carried out
in extended precision on the same float64 inputs — the yardstick the float64 arithmetic's own error is measured with."""
import numpy as np

import range_image_ref

DBL_EPSILON = 2.0 ** -52
TIME_TH = 0.5  # PoseInterp's time_th


def quat_to_R(q):
    """Eigen's toRotationMatrix of quaternions [..., 4] (xyzw) → [..., 3, 3], in q's dtype."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two, one = q.dtype.type(2), q.dtype.type(1)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3), q.dtype)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = one - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, one - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, one - (txx + tyy)
    return R


def pose_at(knot_times, knot_poses, q, dtype=np.float64):
    """The poses [n, 7] at the times q [n] of a track knot_times [K], knot_poses [K, 7]."""
    t, p = np.asarray(knot_times, dtype), np.asarray(knot_poses, dtype).reshape(-1, 7)
    q = np.atleast_1d(np.asarray(q, dtype))
    K, one = len(t), dtype(1)
    j = np.clip(np.searchsorted(t, q, side="left") - 1, 0, K - 2)  # knots with t < q, less one: the first j with t[j] < q <= t[j+1]
    a, b = p[j], p[j + 1]
    dt = t[j + 1] - t[j]
    with np.errstate(all="ignore"):
        s = (q - t[j]) / dt
        d = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]
        ad = np.abs(d)
        lin = ad >= one - dtype(DBL_EPSILON)
        th = np.arccos(np.where(lin, dtype(0), ad))
        st = np.sin(th)
        s0 = np.where(lin, one - s, np.sin((one - s) * th) / st)
        s1 = np.where(lin, s, np.sin(s * th) / st)
        s1 = np.where(d < 0, -s1, s1)
        out = np.empty((len(q), 7), dtype)
        out[:, :4] = s0[:, None] * a[:, :4] + s1[:, None] * b[:, :4]
        out[:, 4:] = a[:, 4:] * (one - s)[:, None] + b[:, 4:] * s[:, None]
    out = np.where((np.abs(dt) < dtype(1e-6))[:, None], a, out)
    return np.where((q > t[K - 1])[:, None], p[K - 1][None, :], out)


def matrices(knot_times, knot_poses, col_time, ref_time, dtype=np.float64):
    """M [n_cols, 3, 4] = [ R_rᵀ·R_c | R_rᵀ·(t_c − t_r) ] of one scan, every dot product summed left to right."""
    pr = pose_at(knot_times, knot_poses, [ref_time], dtype)[0]
    pc = pose_at(knot_times, knot_poses, col_time, dtype)
    Rr, Rc = quat_to_R(pr[:4]), quat_to_R(pc[:, :4])
    d = pc[:, 4:] - pr[4:]
    M = np.empty((len(pc), 3, 4), dtype)
    for r in range(3):
        for c in range(3):
            M[:, r, c] = (Rr[0, r] * Rc[:, 0, c] + Rr[1, r] * Rc[:, 1, c]) + Rr[2, r] * Rc[:, 2, c]
        M[:, r, 3] = (Rr[0, r] * d[:, 0] + Rr[1, r] * d[:, 1]) + Rr[2, r] * d[:, 2]
    return M


def refused(knot_times, col_time, ref_time):
    """The header's time refusals for one scan."""
    t, q = np.asarray(knot_times, np.float64), np.append(np.asarray(col_time, np.float64), ref_time)
    return bool(q.min() < t[0] or q.max() - t[-1] > TIME_TH)


def survivors(model, image):
    """(raw points [n, 4] float32, rings [n] uint8, columns [n]) of one image: range_image_ref.decode's survivors and the column each
    came from (the keep rule restated on the cell grid; checked against decode's rings)."""
    pts, rings = range_image_ref.decode(model, image)
    F = np.float32
    n_rings, n_cols = int(model.n_rings), int(model.n_cols)
    k = np.ascontiguousarray(image, dtype=np.uint16).reshape(n_rings, n_cols)
    cos_az, sin_az = (np.asarray(t, F).reshape(-1, n_cols) for t in (model.cos_az, model.sin_az))
    with np.errstate(all="ignore"):
        r = k.astype(F) * F(model.range_scale)
        h = r * np.asarray(model.cos_el, F).reshape(n_rings, 1)
        x, y, z = h * cos_az, h * sin_az, r * np.asarray(model.sin_el, F).reshape(n_rings, 1)
        keep = (k != 0) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(np.sqrt((x * x + y * y) + z * z) < F(model.min_range))
    g, c = np.nonzero(keep)
    assert np.array_equal(g.astype(np.uint8), rings)
    return pts, rings, c


def apply(pts, cols, mats):
    """locgpu_cloud_transform's arithmetic with each point's column matrix: per row (float)(((m0·x + m1·y) + m2·z) + m3) in float64,
    the w lane carried. pts [n, 4] float32, cols [n], mats [n_cols, 3, 4] float64."""
    m = np.asarray(mats, np.float64)[cols]
    x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
    out = pts.copy()
    for r in range(3):
        out[:, r] = (((m[:, r, 0] * x + m[:, r, 1] * y) + m[:, r, 2] * z) + m[:, r, 3]).astype(np.float32)
    return out
