"""The solve stage that ends every Gauss–Newton iteration (csrc/icp_fit.hip: gn_solve_kernel, loam_solve_kernel, sum_partials_kernel;
csrc/device_math.hpp: lu6_det_solve_reg, se3_apply_update, quat_to_R; the host twin locgpu_gn_update) restated as plain Python.
Nothing here calls the library under test, and nothing here calls the oracle.

    reduce_f64 / reduce_ld   the sum of a scan's block partials: float64 in the documented order — chunk c takes rows c, c + 8, …, 32 loads
                             a round (so 256 rows a round, rows past the end count as 0.0), the eight chunk sums then added in order —
                             and the plain long-double sum of the same rows
    lu6                      the 6×6 partial-pivot LU (Eigen's fixed-size determinant() / inverse(), icp_registration.cpp:210,364) in
                             Python floats, operation for operation; also returns the pivot row of every step and the steps whose pivot
                             was zero
    gn_step / loam_step      the rules per method as plain code: ICP (icp_registration.cpp:204-211, 362-375; P2P's /16 :287), direct NDT
                             (ndt_registration.cpp:435-459), incremental NDT (:349-353), LOAM (loam_registration.cpp:47-90)
    apply_update_f64, quat_to_R, norm6   Sophus SO3::exp · quaternion product · first-order renormalisation, Eigen's toRotationMatrix
                             and dx.norm() in float64, in the associations the reference's binary uses
    apply_update_ld          the same update in numpy.longdouble (64-bit mantissa on x86-64)

Python's float is IEEE binary64 and +, −, ×, ÷ and math.sqrt round correctly, so the float64 parts are what a C compiler without
contraction makes of the same expressions; math.sin / math.cos are the C library's."""
import collections
import math

import numpy as np

LD = np.longdouble
ACC_W, HB_W, LOAM_HB_W = 32, 44, 46
P2P, P2LINE, P2PLANE, NDT_DIRECT, NDT_INC, P2PLANE_MAP = 0, 1, 2, 3, 4, 5
METHODS = (P2P, P2LINE, P2PLANE, NDT_DIRECT, NDT_INC, P2PLANE_MAP)
CHUNKS, FLIGHT = 8, 32
TAYLOR_BELOW = 1e-10


# ------------------------------------------------------------------------------------------------------------------- reduction
def reduce_f64(rows):
    """rows [blocks_per_scan, 32] → the 28 column totals (21 H upper, 6 B, effective_num) in the kernel's order; the spare columns are
    never read."""
    rows = np.asarray(rows, dtype=np.float64)
    n = len(rows)
    zero = np.zeros(28)
    s = np.zeros((CHUNKS, 28))
    for c in range(CHUNKS):
        for b in range(c, n, CHUNKS * FLIGHT):
            for u in range(FLIGHT):
                idx = b + u * CHUNKS
                s[c] = s[c] + (rows[idx, :28] if idx < n else zero)
    t = s[0].copy()
    for c in range(1, CHUNKS):
        t = t + s[c]
    return t


def reduce_ld(rows):
    """The same 28 totals summed in long double, and Σ|row| per column (what the derived bound of the tests scales with)."""
    r = np.asarray(rows, dtype=np.float64)[:, :28].astype(LD)
    return r.sum(axis=0), np.abs(r).sum(axis=0)


def pack_row(H, B, eff, spare=float("nan")):
    """One block partial [32]: H's upper triangle row by row, B, effective_num, four spare doubles."""
    H = np.asarray(H, dtype=np.float64).reshape(6, 6)
    row = np.full(ACC_W, spare, dtype=np.float64)
    o = 0
    for i in range(6):
        for j in range(i, 6):
            row[o] = H[i, j]
            o += 1
    row[21:27] = np.asarray(B, dtype=np.float64)
    row[27] = float(eff)
    return row


def unpack(tot):
    """28 totals → (H as 6 lists of 6 floats, mirrored, B as 6 floats, effective_num as the C cast (long long) makes it)."""
    H = [[0.0] * 6 for _ in range(6)]
    o = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = float(tot[o])
            o += 1
    return H, [float(v) for v in tot[21:27]], math.trunc(float(tot[27]))


# -------------------------------------------------------------------------------------------------------------------------- LU
Lu = collections.namedtuple("Lu", "det x pivots zero_steps")


def lu6(H, b):
    """det(H) and, where it is not zero, x with H x = b (zeros otherwise: the callers start from dx = 0). pivots[k]: the row swapped
    into place at step k; zero_steps: the steps whose pivot was 0.0 (`continue`: no elimination)."""
    a = [[float(H[r][c]) for c in range(6)] for r in range(6)]
    perm = list(range(6))
    det = 1.0
    pivots, zero_steps = [], []
    for k in range(6):
        piv, best = k, abs(a[k][k])
        for r in range(k + 1, 6):
            v = abs(a[r][k])
            if v > best:
                best, piv = v, r
        pivots.append(piv)
        if piv != k:
            a[k], a[piv] = a[piv], a[k]
            perm[k], perm[piv] = perm[piv], perm[k]
            det = -det
        d = a[k][k]
        det *= d
        if d == 0.0:
            zero_steps.append(k)
            continue
        for r in range(k + 1, 6):
            f = a[r][k] / d
            a[r][k] = f
            for c in range(k + 1, 6):
                a[r][c] -= f * a[k][c]
    x = [0.0] * 6
    if det == 0.0:
        return Lu(det, x, pivots, zero_steps)
    y = [0.0] * 6
    for i in range(6):
        s = float(b[perm[i]])
        for j in range(i):
            s -= a[i][j] * y[j]
        y[i] = s
    for i in range(5, -1, -1):
        s = y[i]
        for j in range(i + 1, 6):
            s -= a[i][j] * x[j]
        x[i] = s / a[i][i]
    return Lu(det, x, pivots, zero_steps)


# ---------------------------------------------------------------------------------------------------------------------- update
def norm6(d):
    """dx.norm(): three packets p0 + (p1 + p2), then low + high."""
    return math.sqrt((d[0] * d[0] + (d[2] * d[2] + d[4] * d[4])) + (d[1] * d[1] + (d[3] * d[3] + d[5] * d[5])))


def norm6_left_to_right(d):
    """The plain running sum — NOT what the library or the reference's binary computes; the tests use it to find a dx on which the
    two associations part."""
    n2 = 0.0
    for v in d:
        n2 += v * v
    return math.sqrt(n2)


Update = collections.namedtuple("Update", "q t taylor renormalised theta")


def apply_update_f64(q, t, dx):
    """pose.so3() = pose.so3() * SO3::exp(dx.head<3>()); pose.translation() += dx.tail<3>() in float64."""
    theta_sq = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]
    theta = math.sqrt(theta_sq)
    taylor = theta < TAYLOR_BELOW
    if taylor:
        theta_po4 = theta_sq * theta_sq
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * theta_po4
    else:
        half = 0.5 * theta
        imag = math.sin(half) / theta
        real = math.cos(half)
    bx, by, bz, bw = imag * dx[0], imag * dx[1], imag * dx[2], real
    ax, ay, az, aw = (float(v) for v in q)
    rx = (ay * bz + aw * bx) - (az * by - ax * bw)
    ry = (ay * bw + aw * by) + (az * bx - ax * bz)
    rz = (aw * bz - ay * bx) + (ax * by + az * bw)
    rw = (aw * bw - ay * by) - (ax * bx + az * bz)
    sq = (rz * rz + rx * rx) + (rw * rw + ry * ry)
    renorm = sq != 1.0
    if renorm:
        scale = 2.0 / (sq + 1.0)
        rx *= scale
        ry *= scale
        rz *= scale
        rw *= scale
    return Update([rx, ry, rz, rw], [float(t[0]) + dx[3], float(t[1]) + dx[4], float(t[2]) + dx[5]], taylor, renorm, theta)


def apply_update_ld(q, t, dx):
    """The same update with every operation in long double, from the same float64 inputs → (q [4], t [3]) long double."""
    d = [LD(float(v)) for v in dx]
    theta_sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    theta = np.sqrt(theta_sq)
    if theta < LD(TAYLOR_BELOW):
        theta_po4 = theta_sq * theta_sq
        imag = LD(0.5) - theta_sq / LD(48) + theta_po4 / LD(3840)
        real = LD(1) - theta_sq / LD(8) + theta_po4 / LD(384)
    else:
        half = LD(0.5) * theta
        imag = np.sin(half) / theta
        real = np.cos(half)
    bx, by, bz, bw = imag * d[0], imag * d[1], imag * d[2], real
    ax, ay, az, aw = (LD(float(v)) for v in q)
    r = np.array([(ay * bz + aw * bx) - (az * by - ax * bw), (ay * bw + aw * by) + (az * bx - ax * bz),
                  (aw * bz - ay * bx) + (ax * by + az * bw), (aw * bw - ay * by) - (ax * bx + az * bz)], dtype=LD)
    sq = (r[2] * r[2] + r[0] * r[0]) + (r[3] * r[3] + r[1] * r[1])
    if sq != LD(1):
        r = r * (LD(2) / (sq + LD(1)))
    return r, np.array([LD(float(t[i])) + d[3 + i] for i in range(3)], dtype=LD)


def quat_to_R(q):
    """Eigen::Quaternion::toRotationMatrix, row-major [9]."""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


# ----------------------------------------------------------------------------------------------------------------------- rules
def make_state(q=(0.0, 0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0), R=None, last_dx_norm=0.0, last_eff=0, iterations=0, converged=0, done=0, status=0):
    q = [float(v) for v in q]
    return dict(q=q, t=[float(v) for v in t], R=quat_to_R(q) if R is None else [float(v) for v in R], last_dx_norm=float(last_dx_norm),
                last_eff=int(last_eff), iterations=int(iterations), converged=int(converged), done=int(done), status=int(status))


def _copy(st):
    return dict(st, q=list(st["q"]), t=list(st["t"]), R=list(st["R"]))


def _hb_row(H, B, eff_values, ok_values):
    return [H[i][j] for i in range(6) for j in range(6)] + list(B) + [float(e) for e in eff_values] + [1.0 if o else 0.0 for o in ok_values]


Step = collections.namedtuple("Step", "lu dx update")  # the factorisation, the dx applied (None: no update) and what the update did


def _update_and_stop(st, dx, eps):
    u = apply_update_f64(st["q"], st["t"], dx)
    st["q"], st["t"] = u.q, u.t
    st["R"] = quat_to_R(u.q)
    st["last_dx_norm"] = norm6(dx)
    if st["last_dx_norm"] < eps:  # strict
        st["converged"] = 1
        st["done"] = 1
    return u


def gn_step(tot, state, method, min_effective_pts, eps, max_iteration, do_update=True):
    """One solve of gn_solve_kernel for one scan: (state after, hb row [44] or None where the kernel writes none, Step or None).
    A finished scan (done != 0) is not touched. The two NDT exits (det(H) == 0 in the direct variant, too few accepted residuals in the
    incremental one) end the alignment whatever do_update says — they are the reference's `return false`."""
    if state["done"]:
        return _copy(state), None, None
    st = _copy(state)
    H, B, eff = unpack(tot)
    lu = lu6(H, B)
    if method == NDT_DIRECT:
        if lu.det == 0.0:  # tested first: `return false` before result_pose is written (ndt cpp:435-436)
            st.update(status=1, done=1, iterations=st["iterations"] + 1, last_eff=eff)
            return st, _hb_row(H, B, [eff], [False]), Step(lu, None, None)
        ok = eff >= min_effective_pts  # else `continue` (ndt cpp:438-441)
    elif method == NDT_INC:
        ok = eff >= min_effective_pts  # no test of det(H): H.inverse() of a singular H leaves dx = 0 here (the oracle's rule)
        if not ok:
            st.update(status=2, done=1, iterations=st["iterations"] + 1, last_eff=eff)
            return st, _hb_row(H, B, [eff], [False]), Step(lu, None, None)
    else:
        ok = eff >= min_effective_pts and not lu.det == 0.0  # icp cpp:204-211
    hb = _hb_row(H, B, [eff], [ok])
    st["last_eff"] = eff
    if not do_update:
        return st, hb, Step(lu, None, None)
    st["iterations"] += 1
    dx = u = None
    if ok:
        dx = [v / 16 for v in lu.x] if method == P2P else list(lu.x)  # dx = H.inverse() / 16 * err (icp cpp:287)
        u = _update_and_stop(st, dx, eps)
    if st["iterations"] >= max_iteration:
        st["done"] = 1
    return st, hb, Step(lu, dx, u)


def loam_step(tot_surf, tot_edge, state, min_effective_pts, eps, max_iteration, do_update=True):
    """One solve of loam_solve_kernel for one scan; a class given as None is switched off (eff 0, ok 1). → (state after, hb row [46] or
    None, Step or None; Step.lu is None where the sum is not factorised)."""
    if state["done"]:
        return _copy(state), None, None
    st = _copy(state)
    eff, ok = [0, 0], [True, True]
    tots = [tot_surf, tot_edge]
    for c in range(2):
        if tots[c] is None:
            continue
        H, B, eff[c] = unpack(tots[c])
        ok[c] = eff[c] >= min_effective_pts[c] and not lu6(H, B).det == 0.0
    z = np.zeros(28)
    total = (z if tot_surf is None else np.asarray(tot_surf, dtype=np.float64)) + (z if tot_edge is None else np.asarray(tot_edge, dtype=np.float64))
    H, B, _ = unpack(total)
    hb = _hb_row(H, B, eff, ok)
    st["last_eff"] = eff[0] + eff[1]
    if not do_update:
        return st, hb, Step(None, None, None)
    st["iterations"] += 1
    if not ok[0] or not ok[1]:  # surface is tested first (loam cpp:53-70)
        st.update(status=3 if not ok[0] else 4, done=1)
        return st, hb, Step(None, None, None)
    lu = lu6(H, B)  # no test of the sum's count (loam cpp:76-79); det == 0: an iteration without an update
    dx = u = None
    if not lu.det == 0.0:
        dx = list(lu.x)
        u = _update_and_stop(st, dx, eps)
    if st["iterations"] >= max_iteration:
        st["done"] = 1
    return st, hb, Step(lu, dx, u)


def host_gn_update(hb, method, min_effective_pts, eps, pose):
    """What locgpu_gn_update must return for one hb row [44] and a pose [7]: (pose after, dx, applied, stop)."""
    H = [[float(hb[6 * i + j]) for j in range(6)] for i in range(6)]
    lu = lu6(H, [float(v) for v in hb[36:42]])
    if not (math.trunc(float(hb[42])) >= min_effective_pts and not lu.det == 0.0):
        return [float(v) for v in pose], [0.0] * 6, False, False
    dx = [v / 16 for v in lu.x] if method == P2P else list(lu.x)
    u = apply_update_f64(pose[:4], pose[4:], dx)
    return u.q + u.t, dx, True, norm6(dx) < eps
