"""The NDT fitness score of include/locgpu.h (locgpu_ndt_fitness) restated with numpy, from a voxel table given as arrays — in the tests
the ORACLE's table (locref.Ndt(...).dump()) — and the oracle's FP64 transform. Nothing here calls the library under test.

For every finite point: qs = T·p, key = trunc toward zero of qs / voxel_size, the voxels key + nearby_grids_ (ndt_registration.cpp:57-58),
res = eᵀ·info·e associated as (eᵀ·info)·e with each sum taken left to right, accepted iff !(isnan(res) || res > res_outlier_th); an
inlier's value is its smallest accepted res; score = mean over the inliers, +inf without one."""
import numpy as np

NEARBY = np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1)], dtype=np.int64)  # nearby_grids_ order
BIAS = 1 << 20  # keys live in (-2^20, 2^20) per axis


def pack(k):
    k = np.asarray(k, dtype=np.int64)
    return ((k[..., 0] + BIAS) << 42) | ((k[..., 1] + BIAS) << 21) | (k[..., 2] + BIAS)


class Table:
    """keys [v, 3] int, mu [v, 3], info [v, 3, 3] (row-major: info[v, r, c])."""

    def __init__(self, keys, mu, info):
        keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
        order = np.argsort(pack(keys), kind="stable")
        self.packed = pack(keys)[order]
        assert len(np.unique(self.packed)) == len(self.packed)
        self.mu = np.asarray(mu, dtype=np.float64).reshape(-1, 3)[order]
        self.info = np.asarray(info, dtype=np.float64).reshape(-1, 3, 3)[order]

    def find(self, keys):
        """Index of every key [..., 3] in the table, -1 where it is absent or out of range."""
        keys = np.asarray(keys, dtype=np.int64)
        ok = (np.abs(keys) < BIAS).all(axis=-1)
        p = pack(np.where(ok[..., None], keys, 0))
        at = np.searchsorted(self.packed, p)
        at = np.minimum(at, max(len(self.packed) - 1, 0))
        hit = ok & (self.packed[at] == p) if len(self.packed) else np.zeros(p.shape, bool)
        return np.where(hit, at, -1)


def keys_of(qs, voxel_size):
    return (np.asarray(qs, dtype=np.float64) * (1.0 / voxel_size)).astype(np.int64)  # float64 → int: truncation toward zero


def residuals_at(table, qs, voxel_size, n_nearby):
    """res [n, n_nearby] of the transformed points qs [n, 3] (FP64); NaN where the voxel is not in the table."""
    qs = np.asarray(qs, dtype=np.float64).reshape(-1, 3)
    k = keys_of(qs, voxel_size)
    vid = table.find(k[:, None, :] + NEARBY[None, :n_nearby, :])
    v = np.maximum(vid, 0)
    if len(table.packed) == 0:
        return np.full(vid.shape, np.nan)
    e = qs[:, None, :] - table.mu[v]
    inf = table.info[v]
    ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
    t0 = (ex * inf[..., 0, 0] + ey * inf[..., 1, 0]) + ez * inf[..., 2, 0]
    t1 = (ex * inf[..., 0, 1] + ey * inf[..., 1, 1]) + ez * inf[..., 2, 1]
    t2 = (ex * inf[..., 0, 2] + ey * inf[..., 1, 2]) + ez * inf[..., 2, 2]
    res = (t0 * ex + t1 * ey) + t2 * ez
    return np.where(vid >= 0, res, np.nan)


def score_from_residuals(res, res_outlier_th, finite_points):
    with np.errstate(invalid="ignore"):
        accept = ~(np.isnan(res) | (res > res_outlier_th))
    best = np.where(accept, res, np.inf).min(axis=1) if res.size else np.zeros(0)
    inl = accept.any(axis=1) if res.size else np.zeros(0, bool)
    n = int(inl.sum())
    return dict(score=float(best[inl].sum() / n) if n else float("inf"), inliers=n, finite_points=int(finite_points))


def residuals(locref, table, scan, pose, voxel_size=1.0, n_nearby=7):
    """res [finite points, n_nearby] of a scan under a pose: the oracle's transform, then residuals_at."""
    p = np.ascontiguousarray(np.asarray(scan)[:, :3], dtype=np.float32)
    p = p[np.isfinite(p).all(axis=1)]
    return residuals_at(table, locref.transform_points(pose, p.astype(np.float64)), voxel_size, n_nearby)


def score(locref, table, scan, pose, voxel_size=1.0, n_nearby=7, res_outlier_th=20.0):
    res = residuals(locref, table, scan, pose, voxel_size, n_nearby)
    return score_from_residuals(res, res_outlier_th, len(res))


def gate_margin(res, res_outlier_th):
    """Smallest |res − res_outlier_th| over the (point, voxel) pairs that were found."""
    r = res[~np.isnan(res)]
    return float(np.abs(r - res_outlier_th).min()) if r.size else float("inf")


def winner(fits, min_inlier_ratio=0.5):
    """The rule of locgpu_*_init_search over a list of fitness dicts: index of the winner, or -1."""
    best = -1
    for i, f in enumerate(fits):
        if f["inliers"] <= 0 or not (f["inliers"] >= min_inlier_ratio * f["finite_points"]):
            continue
        if best < 0 or f["score"] < fits[best]["score"]:
            best = i
    return best
