"""CPU restatement of the map-plane mode (include/locgpu.h, LOCGPU_P2PLANE_MAP), composed from oracle pieces only:
the oracle's KD-tree (exact 5-NN for the table, the caller's k = 1 search for the queries), its fit_plane, its FP64 transform,
its 6×6 LU and its SE3 update; numpy only for J, H and B in FP64. A helper module, not a conftest: tests import it."""
import numpy as np

PLANE_GATE = 1e-2  # all five (n3·p + d)² <= 1e-2 (math_utils.h:112-136)


def _leaf_mask(tree, n_points):
    """Points that are leaves of the reference tree (the degenerate-split rule drops the others)."""
    _, _, pidx = tree.dump()
    mask = np.zeros(n_points, dtype=bool)
    mask[pidx[pidx >= 0]] = True
    return mask


def plane_table(locref, tree, map_xyz):
    """The table, rows by original point index: dict(n4 [n, 4] f64, valid [n] bool, leaf [n] bool, nn [n, 5] int32 (-1 without),
    err2 [n, 5] f64 — the five squared plane errors of the oracle's fit, numpy arithmetic)."""
    m = np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, :3])
    n = len(m)
    leaf = _leaf_mask(tree, n)
    n4 = np.zeros((n, 4))
    valid = np.zeros(n, dtype=bool)
    nn = np.full((n, 5), -1, dtype=np.int32)
    err2 = np.full((n, 5), np.inf)
    if tree.num_leaves >= 5:
        rows = np.flatnonzero(leaf)
        nn[rows] = tree.knn(m[rows], k=5, approximate=False)
        for i in rows:
            pts = m[nn[i]].astype(np.float64)
            ok, v = locref.fit_plane(pts)
            n4[i] = v
            valid[i] = ok
            e = pts @ v[:3] + v[3]
            err2[i] = e * e
    return dict(n4=n4, valid=valid, leaf=leaf, nn=nn, err2=err2)


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def hb(locref, tree, table, scan, pose, max_plane_distance=0.1, min_effective_pts=10, approximate=True, alpha=0.1):
    """One evaluation of H, B at `pose` (icp_registration.cpp:161-213 with the fit replaced by the look-up).
    Returns (ok, H [6, 6], B [6], effective_num)."""
    pose = np.asarray(pose, dtype=np.float64)
    p = np.ascontiguousarray(np.asarray(scan, dtype=np.float32)[:, :3])
    q = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    qs = locref.transform_points(pose, q)
    idx = tree.knn(qs.astype(np.float32), k=1, approximate=approximate, alpha=alpha)[:, 0]
    has = idx >= 0
    use = has & table["valid"][np.where(has, idx, 0)]
    eff = int(use.sum())
    q, qs, n4 = q[use], qs[use], table["n4"][idx[use]]
    n3 = n4[:, :3]
    dis = (n3 * qs).sum(axis=1) + n4[:, 3]
    keep = ~(np.abs(dis) > max_plane_distance)
    q, n3, dis = q[keep], n3[keep], dis[keep]
    R = quat_to_R(pose[:4])
    nR = -(n3 @ R)  # rows: -n3ᵀ·R
    J = np.empty((len(q), 6))
    # row·hat(q) with hat(q) = [[0, -qz, qy], [qz, 0, -qx], [-qy, qx, 0]], spelled out
    J[:, 0] = nR[:, 1] * q[:, 2] - nR[:, 2] * q[:, 1]
    J[:, 1] = nR[:, 2] * q[:, 0] - nR[:, 0] * q[:, 2]
    J[:, 2] = nR[:, 0] * q[:, 1] - nR[:, 1] * q[:, 0]
    J[:, 3:] = n3
    H = J.T @ J
    B = -(J.T @ dis)
    det, _ = locref.lu6(H, B)
    ok = eff >= min_effective_pts and not det == 0.0
    return bool(ok), H, B, eff


def align(locref, tree, table, scan, init_pose, max_iteration=20, eps=1e-2, **kw):
    """AlignP2Plane's loop (icp_registration.cpp:345-381) over hb(). Returns dict(pose, iters, converged, eff)."""
    pose = np.asarray(init_pose, dtype=np.float64).copy()
    iters, converged, eff = 0, False, 0
    for _ in range(max_iteration):
        ok, H, B, eff = hb(locref, tree, table, scan, pose, **kw)
        iters += 1
        if not ok:
            continue
        _, dx = locref.lu6(H, B)
        pose = locref.apply_update(pose, dx)
        if np.linalg.norm(dx) < eps:
            converged = True
            break
    return dict(pose=pose, iters=iters, converged=converged, eff=eff)


def excluded_rows(table, map_xyz, gate_tol=1e-9, sv_gap=1e-6):
    """The two exceptions of the table comparison: (near_gate, ill) boolean masks over the points. near_gate: a squared error of the
    oracle's fit lies within gate_tol of the validity gate; ill: the two smallest singular values of the 5×4 matrix are closer than
    sv_gap of the largest (the null vector itself is ill-conditioned there)."""
    m = np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, :3]).astype(np.float64)
    n = len(m)
    rows = np.flatnonzero(table["leaf"] & (table["nn"][:, 0] >= 0))
    near = np.zeros(n, dtype=bool)
    ill = np.zeros(n, dtype=bool)
    if len(rows):
        near[rows] = (np.abs(table["err2"][rows] - PLANE_GATE) <= gate_tol).any(axis=1)
        A = np.concatenate([m[table["nn"][rows]], np.ones((len(rows), 5, 1))], axis=2)
        sv = np.linalg.svd(A, compute_uv=False)
        ill[rows] = (sv[:, 2] - sv[:, 3]) <= sv_gap * sv[:, 0]
    return near, ill
