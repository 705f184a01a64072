"""The per-point terms of one ICP Gauss–Newton iteration (icp_registration.cpp:57-213; oracle/locref.cpp HB_P2P, HB_P2Line, HB_P2Plane)
and of the map-plane mode restated in mpmath at 60 digits. Nothing here calls the library under test, and nothing here
calls the oracle: the neighbour lists are an INPUT (in the tests: the oracle tree's answer to the oracle's own FP64-transformed point
cast to float), so the search is not part of what is compared.

For every source point q (float32, exact in mpmath): qs = R·q + t with R the pose quaternion's rotation matrix (rotation(), the
formula of ndt_hb_ref.rotation), then per method

    P2P       p = the nearest neighbour, e = p − qs, refused iff e·e > max_nn_distance (squared against unsquared, as the reference
              has it); effective_num counts the ACCEPTED points; J = [R·hat(q)/16 | −I3]; a non-finite source point is no query.
    P2LINE    p0 = the mean of the five neighbours, d = the dominant right singular vector of the centred 5×3 matrix; not fitted iff
              some |d×(p_j − p0)|² > max_line_distance (squared against unsquared); effective_num counts the FITTED points;
              e = d×(qs − p0), refused iff |e| > max_line_distance (the norm); J = [−hat(d)·R·hat(q) | hat(d)].
    P2PLANE   n4 = the right singular vector of the smallest singular value of the 5×4 matrix [x y z 1] (a unit 4-vector: n3, its
              first three components, is NOT a unit vector); not fitted iff some (n3·p_j + n4[3])² > 1e-2; effective_num counts the
              FITTED points (before the residual gate); dis = n3·qs + n4[3], refused iff |dis| > max_plane_distance;
              J = [−n3ᵀ·R·hat(q) | n3ᵀ].
    MAPPLANE  the P2PLANE row with n4 = the table row of the nearest neighbour in place of the fit (fitted iff that row is valid).

H = JᵀJ, B = −Jᵀ·e per accepted point. The sign of n4 and of d is free and cancels in H and B.

Conditioning. The error of a computed singular vector grows with the reciprocal gap of its singular value: κ = σ1/(σ3 − σ4) of the
5×4 matrix (plane), κ_line = σ1/(σ1 − σ2) of the centred 5×3 matrix (line); κ = 1 for P2P and the map-plane look-up. A per-point
error is therefore measured in units of u·κ, u = 2^-53 (in_units()).

Results leave mpmath as pairs of doubles (hi, lo), hi + lo holding 32 digits, so that nothing is lost to the conversion."""
import numpy as np
from mpmath import mp, mpf

DPS = 60
U = 2.0 ** -53
P2P, P2LINE, P2PLANE, MAPPLANE = 0, 1, 2, 5
PLANE_FIT_GATE = 1e-2  # math_utils.h:112-136
RANK_REL = 1e-26       # a squared singular value at most this share of the largest counts as zero (the rank rule's threshold)
DEFAULTS = dict(max_nn_distance=1.0, max_plane_distance=0.1, max_line_distance=0.5)
N_GATES = {P2P: 1, P2LINE: 6, P2PLANE: 6, MAPPLANE: 1}


def rotation(pose):
    """Eigen::Quaternion::toRotationMatrix of the pose's quaternion (xyzw), 3×3 list of mpf."""
    x, y, z, w = (mpf(float(v)) for v in np.asarray(pose, dtype=np.float64)[:4])
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def _hat(v):
    o = mpf(0)
    return [[o, -v[2], v[1]], [v[2], o, -v[0]], [-v[1], v[0], o]]


def _mul(a, b):
    return [[sum(a[r][k] * b[k][c] for k in range(len(b))) for c in range(len(b[0]))] for r in range(len(a))]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _eig_sorted(g):
    """Eigenvalues (ascending) and eigenvectors (list of vectors) of the symmetric matrix g (list of lists of mpf)."""
    E, Q = mp.eigsy(mp.matrix(g))
    n = len(g)
    order = sorted(range(n), key=lambda i: E[i])
    return [E[i] for i in order], [[Q[r, i] for r in range(n)] for i in order]


def plane_vector(nb):
    """nb: five points (lists of three mpf). Returns (n4 [4 mpf], kappa (mpf, inf without a gap), rank_deficient (bool): fewer than
    three squared singular values above RANK_REL of the largest — the null space has two or more dimensions and n4 is arbitrary)."""
    A = [[p[0], p[1], p[2], mpf(1)] for p in nb]
    G = [[sum(A[i][r] * A[i][c] for i in range(5)) for c in range(4)] for r in range(4)]
    E, V = _eig_sorted(G)
    sv = [mp.sqrt(e) if e > 0 else mpf(0) for e in E]
    gap = sv[1] - sv[0]
    kappa = sv[3] / gap if gap > 0 else mpf("inf")
    rank = sum(1 for e in E if e > mpf(RANK_REL) * E[3])
    return V[0], kappa, rank < 3


def line_vector(nb):
    """nb: five points. Returns (p0, d [3 mpf], kappa_line)."""
    p0 = [(nb[0][c] + nb[1][c] + nb[2][c] + nb[3][c] + nb[4][c]) / 5 for c in range(3)]
    C = [[p[c] - p0[c] for c in range(3)] for p in nb]
    G = [[sum(C[i][r] * C[i][c] for i in range(5)) for c in range(3)] for r in range(3)]
    E, V = _eig_sorted(G)
    sv = [mp.sqrt(e) if e > 0 else mpf(0) for e in E]
    gap = sv[2] - sv[1]
    return p0, V[2], (sv[2] / gap if gap > 0 else mpf("inf"))


def _rel(x, gate):
    """Distance of the gated quantity x to its gate, relative to the gate."""
    return float(abs(x - gate) / gate)


def _split(x):
    hi = float(x)
    return hi, float(x - mpf(hi))


def _mp_point(p):
    return [mpf(float(p[0])), mpf(float(p[1])), mpf(float(p[2]))]


def plane_table(map_xyz, nn):
    """The exact plane of every listed neighbourhood: nn [m, 5] indices into map_xyz (float32; a row with a negative index has no
    plane). Returns dict(n4, n4_lo [m, 4], valid [m] bool (all five (n3·p + d)² <= 1e-2), kappa [m], rank_deficient [m] bool,
    gates [m, 5] (relative distance of each squared error to 1e-2; inf without a plane))."""
    m = np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, :3])
    nn = np.asarray(nn)
    k = len(nn)
    out = dict(n4=np.zeros((k, 4)), n4_lo=np.zeros((k, 4)), valid=np.zeros(k, bool), kappa=np.full(k, np.inf), rank_deficient=np.zeros(k, bool),
               gates=np.full((k, 5), np.inf))
    with mp.workdps(DPS):
        gate = mpf(PLANE_FIT_GATE)
        for i in range(k):
            if (nn[i] < 0).any():
                continue
            nb = [_mp_point(m[j]) for j in nn[i]]
            n4, kappa, rd = plane_vector(nb)
            err2 = [(_dot(n4[:3], p) + n4[3]) ** 2 for p in nb]
            out["valid"][i] = not any(e > gate for e in err2)
            out["gates"][i] = [_rel(e, gate) for e in err2]
            out["kappa"][i] = float(kappa)
            out["rank_deficient"][i] = rd
            for c in range(4):
                out["n4"][i, c], out["n4_lo"][i, c] = _split(n4[c])
    return out


def per_point(method, map_xyz, nn, scan, pose, planes=None, **opts):
    """Per source point of `scan` (float32 [n, ≥3]) under `pose` (7 doubles, quaternion xyzw + t) against the neighbours nn [n, k]
    (indices into map_xyz, k = 1 for P2P and MAPPLANE, 5 for P2LINE and P2PLANE; a negative first index = no neighbours).
    planes (MAPPLANE): (n4 [n_map, 4] float64, valid [n_map] bool). opts: max_nn_distance, max_plane_distance, max_line_distance.

    Returns dict of H, H_lo [n, 6, 6], B, B_lo [n, 6] (hi + lo), fitted, accepted [n] bool, kappa [n] (float64; inf where the fit has
    no gap), vec, vec_lo [n, 4] (n4 of P2PLANE; d in the first three of P2LINE; the sign is free), rank_deficient [n] bool (P2PLANE),
    gates [n, N_GATES[method]]: the distance of every gated quantity to its gate, relative to the gate (inf where not evaluated):
    P2P e·e; P2LINE the five |d×(p_j − p0)|², then |e|; P2PLANE the five squared plane errors, then |dis|; MAPPLANE |dis|."""
    o = dict(DEFAULTS)
    o.update(opts)
    m = np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, :3])
    s = np.ascontiguousarray(np.asarray(scan, dtype=np.float32)[:, :3])
    nn = np.asarray(nn).reshape(len(s), -1)
    n = len(s)
    out = dict(H=np.zeros((n, 6, 6)), H_lo=np.zeros((n, 6, 6)), B=np.zeros((n, 6)), B_lo=np.zeros((n, 6)), fitted=np.zeros(n, bool),
               accepted=np.zeros(n, bool), kappa=np.ones(n), vec=np.zeros((n, 4)), vec_lo=np.zeros((n, 4)), rank_deficient=np.zeros(n, bool),
               gates=np.full((n, N_GATES[method]), np.inf))
    with mp.workdps(DPS):
        R = rotation(pose)
        t = [mpf(float(v)) for v in np.asarray(pose, dtype=np.float64)[4:]]
        g_nn, g_plane, g_line = mpf(o["max_nn_distance"]), mpf(o["max_plane_distance"]), mpf(o["max_line_distance"])
        g_fit = mpf(PLANE_FIT_GATE)
        for i in range(n):
            if nn[i, 0] < 0 or not np.isfinite(s[i]).all():  # no query (every per-point input of the tests is finite)
                continue
            q = _mp_point(s[i])
            qs = [_dot(R[r], q) + t[r] for r in range(3)]
            J, e = None, None
            if method == P2P:
                p = _mp_point(m[nn[i, 0]])
                e = [p[c] - qs[c] for c in range(3)]
                dis2 = _dot(e, e)
                out["gates"][i, 0] = _rel(dis2, g_nn)
                if dis2 > g_nn:
                    continue
                out["fitted"][i] = True  # effective_num++ behind the gate
                Rh = _mul(R, _hat(q))
                J = [[Rh[r][c] / 16 for c in range(3)] + [mpf(-1) if r == c else mpf(0) for c in range(3)] for r in range(3)]
            elif method == P2LINE:
                nb = [_mp_point(m[j]) for j in nn[i]]
                p0, d, kappa = line_vector(nb)
                out["kappa"][i] = float(kappa)
                for c in range(3):
                    out["vec"][i, c], out["vec_lo"][i, c] = _split(d[c])
                c2 = []
                for p in nb:
                    cr = _cross(d, [p[c] - p0[c] for c in range(3)])
                    c2.append(_dot(cr, cr))
                out["gates"][i, :5] = [_rel(v, g_line) for v in c2]
                if any(v > g_line for v in c2):
                    continue
                out["fitted"][i] = True
                e = _cross(d, [qs[c] - p0[c] for c in range(3)])
                nrm = mp.sqrt(_dot(e, e))
                out["gates"][i, 5] = _rel(nrm, g_line)
                if nrm > g_line:
                    continue
                hd = _hat(d)
                A = _mul(_mul(hd, R), _hat(q))
                J = [[-A[r][c] for c in range(3)] + [hd[r][c] for c in range(3)] for r in range(3)]
            else:
                if method == P2PLANE:
                    nb = [_mp_point(m[j]) for j in nn[i]]
                    n4, kappa, rd = plane_vector(nb)
                    out["kappa"][i] = float(kappa)
                    out["rank_deficient"][i] = rd
                    for c in range(4):
                        out["vec"][i, c], out["vec_lo"][i, c] = _split(n4[c])
                    err2 = [(_dot(n4[:3], p) + n4[3]) ** 2 for p in nb]
                    out["gates"][i, :5] = [_rel(v, g_fit) for v in err2]
                    if any(v > g_fit for v in err2):
                        continue
                else:
                    if not planes[1][nn[i, 0]]:
                        continue
                    n4 = [mpf(float(v)) for v in planes[0][nn[i, 0]]]
                    for c in range(4):
                        out["vec"][i, c] = float(n4[c])
                out["fitted"][i] = True  # effective_num++ before the residual gate (icp cpp:184)
                n3 = n4[:3]
                dis = _dot(n3, qs) + n4[3]
                out["gates"][i, -1] = _rel(abs(dis), g_plane)
                if abs(dis) > g_plane:
                    continue
                nR = [-(n3[0] * R[0][c] + n3[1] * R[1][c] + n3[2] * R[2][c]) for c in range(3)]
                hq = _hat(q)
                J = [[sum(nR[k] * hq[k][c] for k in range(3)) for c in range(3)] + list(n3)]
                e = [dis]
            out["accepted"][i] = True
            for a in range(6):
                for b in range(a, 6):
                    h = sum(J[r][a] * J[r][b] for r in range(len(J)))
                    out["H"][i, a, b], out["H_lo"][i, a, b] = _split(h)
                    out["H"][i, b, a], out["H_lo"][i, b, a] = out["H"][i, a, b], out["H_lo"][i, a, b]
                out["B"][i, a], out["B_lo"][i, a] = _split(-sum(J[r][a] * e[r] for r in range(len(J))))
    return out


def near_gate(pp, rel=1e-9):
    """Points [n] bool with a gated quantity within `rel` (relative) of its gate: a different rounding of the same quantity may fall on
    the other side there."""
    return (pp["gates"] <= rel).any(axis=1)


def totals(pp):
    """(H [6, 6], B [6], effective_num, accepted) of a whole scan: the per-point terms summed in long double, rounded to double."""
    LD = np.longdouble
    H = (pp["H"].astype(LD) + pp["H_lo"].astype(LD)).sum(axis=0)
    B = (pp["B"].astype(LD) + pp["B_lo"].astype(LD)).sum(axis=0)
    return H.astype(np.float64), B.astype(np.float64), int(pp["fitted"].sum()), int(pp["accepted"].sum())


def point_errors(Hg, Bg, pp):
    """Per point, the NDT scaling (ndt_hb_ref.point_errors): (|H − H_ref| / max|H_ref|, |B − B_ref| / max(|B_ref|, sqrt(max|H_ref|))),
    the worst entry each, float64 [n]. A refused point has H_ref = 0: there any non-zero entry is an error of 1 (absolute)."""
    Hr, Br = pp["H"], pp["B"]
    hs = np.abs(Hr).max(axis=(1, 2))
    bs = np.maximum(np.abs(Br).max(axis=1), np.sqrt(hs))
    hs = np.where(hs > 0, hs, 1.0)
    bs = np.where(bs > 0, bs, 1.0)
    # (got − hi) is exact where the two are close (Sterbenz), so the difference to hi + lo is formed without a rounding of the reference
    eh = np.abs((np.asarray(Hg, dtype=np.float64) - Hr) - pp["H_lo"]).max(axis=(1, 2)) / hs
    eb = np.abs((np.asarray(Bg, dtype=np.float64) - Br) - pp["B_lo"]).max(axis=1) / bs
    return eh, eb


def vector_errors(got, vec, vec_lo):
    """|got − ref| per row (largest component), up to the free sign; got, vec, vec_lo [n, w]."""
    got = np.asarray(got, dtype=np.float64)
    plus = np.abs((got - vec) - vec_lo).max(axis=1)
    minus = np.abs((got + vec) + vec_lo).max(axis=1)
    return np.minimum(plus, minus)


def in_units(err, kappa):
    """err / (u·κ)."""
    return np.asarray(err) / (U * np.asarray(kappa))
