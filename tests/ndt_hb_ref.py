"""The per-point sums of one NDT Gauss–Newton iteration (ndt_registration.cpp:399-433 direct, :286-347 incremental) restated in
numpy.longdouble, from a voxel table given as arrays — in the tests the ORACLE's table (locref.Ndt(...).dump()) — the float32 scan and
an FP64 pose. Nothing here calls the library under test, and nothing here calls the oracle.

For every source point q: qs = R·q + t, key = trunc toward zero of qs / voxel_size, the voxels key + nearby_grids_ (:57-58) in that
order; for every voxel found e = qs − μ, res = eᵀ·info·e, accepted iff !(isnan(res) || res > res_outlier_th). With J = [−R·hat(q) | I3]:

    direct       H += JᵀJ          B += −Jᵀe          per accepted voxel (not weighted by info)
    incremental  H += Jᵀ·info·J    B += −Jᵀ·info·e    per accepted voxel

The sums are formed entry by entry in long double (64-bit mantissa on x86-64: 2^-64 per operation against the 2^-53 of the FP64 code
under test), with no regrouping: per point Σ over voxels of the full 6×6 product."""
import numpy as np

import ndt_score_ref as score_ref

LD = np.longdouble
NEARBY = score_ref.NEARBY
Table = score_ref.Table


def rotation(pose):
    """Eigen::Quaternion::toRotationMatrix of the pose's quaternion (xyzw), long double [3, 3]."""
    x, y, z, w = (LD(v) for v in np.asarray(pose, dtype=np.float64)[:4])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=LD)


def hat(q):
    """Sophus SO3::hat of every row of q [n, 3] → [n, 3, 3]."""
    o = np.zeros(len(q), dtype=LD)
    return np.stack([np.stack([o, -q[:, 2], q[:, 1]], -1), np.stack([q[:, 2], o, -q[:, 0]], -1), np.stack([-q[:, 1], q[:, 0], o], -1)], -2)


def per_point(table, scan, pose, voxel_size=1.0, n_nearby=7, res_outlier_th=20.0, weighted=False):
    """Per source point of `scan` (float32 [n, ≥3]) under `pose`: dict of
    H [n, 6, 6], B [n, 6] (long double), n_acc [n] (accepted voxels), res [n, n_nearby] (long double, NaN where the voxel is not in
    the table or the point has no key), accept [n, n_nearby]."""
    q = np.ascontiguousarray(np.asarray(scan)[:, :3], dtype=np.float32).astype(LD)
    n = len(q)
    R = rotation(pose)
    t = np.asarray(pose, dtype=np.float64)[4:].astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        qs = q @ R.T + t
        scaled = qs * (LD(1.0) / LD(voxel_size))
        keyed = np.isfinite(scaled).all(axis=1) & (np.abs(scaled) < 2 * score_ref.BIAS).all(axis=1)  # the rest has no voxel, whatever its key would be
    k = np.trunc(np.where(keyed[:, None], scaled, 0)).astype(np.int64)
    vid = table.find(k[:, None, :] + NEARBY[None, :n_nearby, :])
    vid = np.where(keyed[:, None], vid, -1)
    v = np.maximum(vid, 0)
    have = len(table.packed) > 0
    mu = table.mu[v].astype(LD) if have else np.zeros(vid.shape + (3,), LD)
    info = table.info[v].astype(LD) if have else np.zeros(vid.shape + (3, 3), LD)
    with np.errstate(invalid="ignore", over="ignore"):
        e = qs[:, None, :] - mu                                      # [n, j, 3]
        ie = np.einsum("njrc,njc->njr", info, e)                     # info·e
        res = np.einsum("njr,njr->nj", e, ie)
        res = np.where(vid >= 0, res, LD("nan"))
        accept = (vid >= 0) & ~(np.isnan(res) | (res > LD(res_outlier_th)))
    J = np.zeros((n, 3, 6), dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        J[:, :, :3] = -np.einsum("rk,nkc->nrc", R, hat(q))
    J[:, :, 3:] = np.eye(3, dtype=LD)
    H = np.zeros((n, 6, 6), dtype=LD)
    B = np.zeros((n, 6), dtype=LD)
    for j in range(vid.shape[1]):
        a = accept[:, j]
        if not a.any():
            continue
        Ja = J[a]
        if weighted:
            W, we = info[a, j], ie[a, j]
        else:
            W, we = np.broadcast_to(np.eye(3, dtype=LD), (int(a.sum()), 3, 3)), e[a, j]
        H[a] += np.einsum("nra,nrs,nsb->nab", Ja, W, Ja)
        B[a] += -np.einsum("nra,nr->na", Ja, we)
    return dict(H=H, B=B, n_acc=accept.sum(axis=1).astype(np.int64), res=res, accept=accept)


def near_gate(res, res_outlier_th, rel=1e-9):
    """Points [n] bool that have a (point, voxel) pair whose residual lies within `rel` (relative) of the gate: a different rounding of
    the same residual may fall on the other side there."""
    with np.errstate(invalid="ignore"):
        return (np.abs(res - LD(res_outlier_th)) <= LD(rel) * LD(res_outlier_th)).any(axis=1)


def totals(pp):
    """(H [6, 6], B [6], accepted pairs) of a whole scan: the per-point terms summed in long double."""
    return pp["H"].sum(axis=0), pp["B"].sum(axis=0), int(pp["n_acc"].sum())


def point_errors(Hg, Bg, pp):
    """Per point: (|H − H_ref| / max|H_ref|, |B − B_ref| / max(|B_ref|, sqrt(max|H_ref|))), the worst entry each, as float64 [n].
    A point without an accepted voxel has H_ref = 0: there any non-zero entry is an error of 1 (absolute)."""
    Hr, Br = pp["H"], pp["B"]
    hs = np.abs(Hr).max(axis=(1, 2))
    bs = np.maximum(np.abs(Br).max(axis=1), np.sqrt(hs))
    hs = np.where(hs > 0, hs, LD(1))
    bs = np.where(bs > 0, bs, LD(1))
    eh = np.abs(np.asarray(Hg).astype(LD) - Hr).max(axis=(1, 2)) / hs
    eb = np.abs(np.asarray(Bg).astype(LD) - Br).max(axis=1) / bs
    return eh.astype(np.float64), eb.astype(np.float64)
