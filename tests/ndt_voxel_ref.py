"""One NDT voxel's record restated in mpmath at 60 digits: what ndt_voxel_record (csrc/ndt_ingest.hpp, the direct table and the voxel
set) and inc_stats_kernel (csrc/ndt_inc.hip, the incremental table) are asked to compute, from the float32 points taken as exact and
in input order. Nothing here calls the library under test, and nothing here calls the oracle.

    mu        the mean
    cov       S = scatter / (n - 1)
    lam, vec  the eigen-pairs of S in descending order (mp.eigsy); vec[k] is the k-th eigenvector
    terms     T_k = v_k v_k^T / max(lam_k, 1e-3 lam_0)                 (ndt_registration.cpp:118-130 with U = V, what S symmetric PSD means)
    direct    T_0 + T_1 + T_2                                          None when lam_0 = 0 (coincident points: the record is not defined)
    inc       (S + 1e-3 I)^-1; one point: mu = p, info = 100 I         (ndt_registration.cpp:185-236, the first-scan branch)
    kappa_c   lam_0 / max(lam_2, 1e-3 lam_0)        the conditioning of the direct record, at most 1000
    kappa_i   (lam_0 + 1e-3) / (lam_2 + 1e-3)       that of the incremental one
    ratio     lam_2 / lam_0 (lam_0 = 0: 0)

The errors are measured as E / (u kappa): E = max|info - ref| / max|ref|, u = 2^-53.

The key rule is restated the way tests/ndt_table_cases.py does it: truncation toward zero of p * (1 / voxel_size) in double."""
import numpy as np
from mpmath import mp, mpf

DPS = 60
U = 2.0 ** -53
CLAMP = mpf(1) / 1000      # lam_1, lam_2 >= 1e-3 lam_0
INC_EPS = mpf(1) / 1000    # the incremental record's + 1e-3 I
FULL_RANK = 1e-13          # a case is full rank iff lam_2 / lam_0 >= this …
DEFICIENT = 1e-20          # … rank-deficient iff <= this, and no designed case may lie between


def keys_of(points, voxel_size=1.0):
    """(pt * inv_voxel).cast<int>(): float32 → double, times 1/voxel_size in double, truncated toward zero → [n, 3] int64."""
    p = np.asarray(points, dtype=np.float32)[:, :3].astype(np.float64)
    return np.trunc(p * (1.0 / float(voxel_size))).astype(np.int64)


def _mat(rows):
    return mp.matrix([[mpf(x) for x in r] for r in rows])


def _outer(v, scale):
    return mp.matrix(3, 3) + mp.matrix([[v[i] * v[j] * scale for j in range(3)] for i in range(3)])


def record(points):
    """The reference record of one voxel holding `points` (float32 [n, 3], n >= 1) → dict, mp numbers (see the module's docstring)."""
    p = np.asarray(points, dtype=np.float32)[:, :3]
    n = len(p)
    assert n >= 1 and np.isfinite(p).all()
    with mp.workdps(DPS):
        rows = [[mpf(float(x)) for x in r] for r in p]
        mu = [sum(r[k] for r in rows) / n for k in range(3)]
        if n == 1:
            return dict(n=1, mu=mu, cov=None, lam=None, vec=None, terms=None, direct=None, inc=mp.eye(3) * 100, kappa_c=None, kappa_i=mpf(1), ratio=None)
        d = [[r[k] - mu[k] for k in range(3)] for r in rows]
        cov = mp.matrix(3, 3)
        for i in range(3):
            for j in range(i, 3):
                cov[i, j] = cov[j, i] = sum(r[i] * r[j] for r in d) / (n - 1)
        ev, Q = mp.eigsy(cov)
        order = sorted(range(3), key=lambda k: -ev[k])
        lam = [ev[k] if ev[k] > 0 else mpf(0) for k in order]  # exact zeros come out as ±1e-60
        vec = [[Q[i, k] for i in range(3)] for k in order]
        inc = (cov + mp.eye(3) * INC_EPS) ** -1
        kappa_i = (lam[0] + INC_EPS) / (lam[2] + INC_EPS)
        if lam[0] == 0:
            return dict(n=n, mu=mu, cov=cov, lam=lam, vec=vec, terms=None, direct=None, inc=inc, kappa_c=None, kappa_i=kappa_i, ratio=mpf(0))
        floor = CLAMP * lam[0]
        terms = [_outer(vec[k], 1 / max(lam[k], floor)) for k in range(3)]
        return dict(n=n, mu=mu, cov=cov, lam=lam, vec=vec, terms=terms, direct=terms[0] + terms[1] + terms[2], inc=inc,
                    kappa_c=lam[0] / max(lam[2], floor), kappa_i=kappa_i, ratio=lam[2] / lam[0])


def rank_class(rec):
    """'full' (lam_2/lam_0 >= 1e-13), 'deficient' (<= 1e-20), 'coincident' (lam_0 = 0), 'single' (one point) or 'band' (between the two
    classes: a designed case may not be there)."""
    if rec["n"] == 1:
        return "single"
    if rec["lam"][0] == 0:
        return "coincident"
    r = float(rec["ratio"])
    return "full" if r >= FULL_RANK else ("deficient" if r <= DEFICIENT else "band")


def rel_err(info, ref):
    """E = max|info - ref| / max|ref| of a float64 [3, 3] against an mp matrix, formed at 60 digits → float."""
    with mp.workdps(DPS):
        a = np.asarray(info, dtype=np.float64)
        num = max(abs(mpf(float(a[i, j])) - ref[i, j]) for i in range(3) for j in range(3))
        den = max(abs(ref[i, j]) for i in range(3) for j in range(3))
        return float(num / den)


def figure(info, ref, kappa):
    """E / (u kappa)."""
    return rel_err(info, ref) / (U * float(kappa))


def asymmetry(info):
    a = np.asarray(info, dtype=np.float64)
    return float(np.abs(a - a.T).max() / np.abs(a).max())


def mu_bound(points):
    """A sequential double sum of n float32 values and one division: |mu - mu_ref| <= (n + 1) u max|p| per axis → float64 [3]."""
    p = np.abs(np.asarray(points, dtype=np.float32)[:, :3].astype(np.float64))
    return (len(p) + 1) * U * p.max(axis=0)


def mu_err(mu, rec):
    """|mu - mu_ref| per axis → float64 [3]."""
    with mp.workdps(DPS):
        return np.array([float(abs(mpf(float(mu[k])) - rec["mu"][k])) for k in range(3)])


def candidates(rec):
    """The two valid direct records of an exactly coplanar voxel: (T0 + T1 + T2, T0 + T1 - T2). lam_2 is rounding noise there, its
    direction is not: the computed U column is +v2 or -v2."""
    t = rec["terms"]
    with mp.workdps(DPS):
        return t[0] + t[1] + t[2], t[0] + t[1] - t[2]


def null_space_checks(info, rec):
    """What any valid record of a voxel with a null space of two dimensions obeys → (e_right, e_left, s_max, finite):
    |info v0 - v0/lam0| and |v0^T info - v0^T/lam0|, worst entry relative to 1/lam0; the largest singular value of info times
    lam0/1000 (at most 1 up to rounding); every entry finite."""
    a = np.asarray(info, dtype=np.float64)
    if not np.isfinite(a).all():
        return np.inf, np.inf, np.inf, False
    with mp.workdps(DPS):
        A = _mat(a.tolist())
        v0 = mp.matrix(rec["vec"][0])
        l0 = rec["lam"][0]
        right = A * v0 - v0 / l0
        left = v0.T * A - v0.T / l0
        e_r = float(max(abs(x) for x in right) * l0)
        e_l = float(max(abs(x) for x in left) * l0)
        s = float(mp.svd_r(A, compute_uv=False)[0] * l0 / 1000)
    return e_r, e_l, s, True


def to_float(m):
    """An mp 3×3 → float64 [3, 3] (nearest)."""
    return np.array([[float(m[i, j]) for j in range(3)] for i in range(3)])
