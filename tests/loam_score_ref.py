"""A numpy restatement of the LOAM matcher's joint fitness score (include/locgpu.h, locgpu_loam_fitness): per enabled class the
definition of locgpu_icp_fitness — queries q = (float32)(T·p) with the product in float64, exact brute-force 1-NN in float32 with the
search's grouping dx² + (dy² + dz²), inliers d² <= (float32)(max_range²), the sum of the inliers' d² in float64 — and then the POOLED
mean (Σ_surf + Σ_edge) / (inliers_surf + inliers_edge), surface first; +inf without an inlier in either class. Test infrastructure:
nothing here calls the library."""
import numpy as np


def quat_transform(pose, pts):
    """T·p in float64 for pose = (qx, qy, qz, qw, tx, ty, tz); the GPU tests pass the oracle's transform_points instead, whose
    rounding order is the library's."""
    x, y, z, w = (float(v) for v in pose[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return pts @ R.T + np.asarray(pose[4:], dtype=np.float64)


def _all_pairs_d2(m, q, block=256):
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    out = np.empty(len(q), np.float32)
    for a in range(0, len(q), block):
        b = q[a:a + block]
        dx, dy, dz = b[:, 0:1] - mx, b[:, 1:2] - my, b[:, 2:3] - mz
        out[a:a + block] = (dx * dx + (dy * dy + dz * dz)).min(axis=1)
    return out


def nn_d2(map_xyz, q, all_pairs=False):
    """float32 squared distance from every query to its exact nearest map point, by brute force. all_pairs: every pair is evaluated.
    Otherwise a query skips the map points that cannot be its nearest: an upper bound u on its answer comes from every 64th map point
    (all of those pairs evaluated), and a point with |dx| > sqrt(u) · (1 + 1e-6) has d² > u whatever its y and z — the float32 d² is
    monotone in the rounded dx² it starts from, and the margin covers the three roundings — so only the slab |dx| <= that is
    evaluated, all of it. Same values, a map of 200 000 points in a fraction of a second (test_loam_score_ref.py compares the two)."""
    m = np.ascontiguousarray(map_xyz, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    if all_pairs or len(m) < 4096:
        return _all_pairs_d2(m, q)
    m = m[np.argsort(m[:, 0], kind="stable")]
    upper = _all_pairs_d2(m[::64], q).astype(np.float64)
    r = np.sqrt(upper) * (1.0 + 1e-6)
    qx, mx = q[:, 0].astype(np.float64), m[:, 0].astype(np.float64)
    lo, hi = np.searchsorted(mx, qx - r, side="left"), np.searchsorted(mx, qx + r, side="right")
    out = np.empty(len(q), np.float32)
    for i in range(len(q)):
        if not np.isfinite(r[i]):  # an overflowed bound: every pair
            lo[i], hi[i] = 0, len(m)
        d = q[i] - m[lo[i]:hi[i]]
        out[i] = (d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])).min()
    return out


def class_sums(map_xyz, scan, pose, max_range, transform=quat_transform):
    """(Σ d² of the inliers [float64], inliers, finite points) of one class; a class that is switched off is scan=None: zeros."""
    if scan is None or len(scan) == 0:
        return 0.0, 0, 0
    p = np.ascontiguousarray(np.asarray(scan)[:, :3], dtype=np.float32)
    p = p[np.isfinite(p).all(axis=1)]  # pcl::isFinite: not a query, not counted
    if len(p) == 0:
        return 0.0, 0, 0
    q = np.asarray(transform(pose, p.astype(np.float64))).astype(np.float32)
    d2 = nn_d2(map_xyz, q)
    inl = d2 <= np.float32(max_range * max_range)
    return float(d2[inl].astype(np.float64).sum()), int(inl.sum()), len(p)


def _fit(s, n, fin):
    return dict(score=s / n if n else float("inf"), inliers=n, finite_points=fin)


def joint_score(edge_map, surf_map, edge, surf, pose, max_range=1.0, transform=quat_transform):
    """[joint, surface, edge] as dicts(score, inliers, finite_points) — the three entries locgpu_loam_fitness reports per pose."""
    ss, ns, fs = class_sums(surf_map, surf, pose, max_range, transform)
    se, ne, fe = class_sums(edge_map, edge, pose, max_range, transform)
    return [_fit(ss + se, ns + ne, fs + fe), _fit(ss, ns, fs), _fit(se, ne, fe)]


def winner(joint, min_inlier_ratio=0.5):
    """The rule of locgpu_loam_init_search over the joint entries: lowest score among those with an inlier and the ratio, ties to the
    lower index; -1 when none qualifies."""
    ok = [i for i, f in enumerate(joint) if f["inliers"] >= 1 and f["inliers"] >= min_inlier_ratio * f["finite_points"]]
    return min(ok, key=lambda i: (joint[i]["score"], i)) if ok else -1
