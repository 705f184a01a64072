"""Inputs and CPU restatements shared by tests/test_fitness_cases_ref.py (CPU) and tests/test_gpu_fitness_points.py (GPU): the fitness
scores of include/locgpu.h (locgpu_icp_fitness, locgpu_ndt_fitness, locgpu_loam_fitness) per point, at the gates and by the row shapes
of the fixed-order sum (csrc/fitness.hip, csrc/ndt_fitness.hip). Nothing here needs a device, and nothing here calls the library under
test except host_tree_depth (the host tree builder, no device).

1. The ICP score per point: brute_d2 is the header's d² by brute force over all map points in float32, dx·dx + (dy·dy + dz·dz); the
   inputs are icp_point_inputs.

2. exact_world: a world in which every quantity of the ICP score is exact. The map is a product grid (65 x 65 x 3 points, 1/2 m apart;
   the host tree of it is 17 levels deep, within the limit of 64); the scan's coordinates are multiples of 1/16 m; the poses are
   half-turns (or the identity) with translations in multiples of 1/16 m, for which se3_apply is exact. Lengths are kept as int64
   integers in units of 1/16 m (Q = 16), squared distances in units of 2^-8 m² (Q2 = 256): every d² is below 2^5 m², so it has at
   most 13 significant bits (exact in float32, products and both sums included), and a sum of up to 2^18 of them has at most 31
   (exact in FP64 in any order). The reference for Σ is an integer sum.

3. The NDT score per point at 60 digits (mpmath): ndt_point_ref, with the scale S of its rounding bound; ndt_point_inputs chooses
   the compared points so that the minimum over the probed voxels matters."""
import ctypes
import math

import numpy as np

import ndt_score_ref

U = 2.0 ** -53
BAR_FACTOR = 8.0       # the project's factor (icp_hb_cases.BAR_FACTOR, ndt_hb_cases.BAR_FACTOR)
GATE_REL = 1e-9        # an NDT residual this close (relative) to res_outlier_th may fall either side of it
KEY_MARGIN = 1e-9      # a qs / voxel_size component this close to an integer may be truncated either way
RES_TH = 20.0          # NdtOptions::res_outlier_th_ default
VOXEL = 1.0            # NdtOptions::voxel_size_ default

# The per-point unit of the NDT score: the worst err / (u·S) of the numpy restatement ndt_score_ref.residuals_at (fed the oracle's FP64
# transform) against the 60-digit value over ndt_point_inputs on the oracle's table, measured and printed by
# test_fitness_cases_ref.py::test_unit_of_the_ndt_restatement, recorded here rounded up and never below 1.
UNIT = 2.5             # measured 2.45

ROW_LENGTHS = (1, 255, 256, 257, 1023, 1024, 1025, 4096, 65536, 65537, 131073)
RAGGED = (131073, 65537, 1025, 1, 0)


# ------------------------------------------------------------------------------------------------ 1. the ICP score per point
def brute_d2(q, map_xyz, chunk=64):
    """float32 [n]: min over ALL map points of dx·dx + (dy·dy + dz·dz) in float32 (KdTree::ComputeDisForLeaf's grouping). A query with
    a non-finite coordinate gives NaN or inf."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    mx, my, mz = (np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, a]) for a in range(3))
    out = np.empty(len(q), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, len(q), chunk):
            c = q[lo:lo + chunk]
            dx, dy, dz = c[:, None, 0] - mx[None, :], c[:, None, 1] - my[None, :], c[:, None, 2] - mz[None, :]
            out[lo:lo + chunk] = (dx * dx + (dy * dy + dz * dz)).min(axis=1)
    return out


def hostile(s):
    """s with NaN / ±inf / 1e30 rows mixed in (the rows of test_gpu_icp_hb._hostile)."""
    h = np.array(s, copy=True)
    nan, inf = np.float32("nan"), np.float32("inf")
    for r, v in {3: (nan, 1, 2), 40: (1, nan, nan), 99: (inf, 0, 0), 100: (0, -inf, 1), 101: (inf, -inf, inf), 200: (1e30, 0, 0), 201: (0, -1e30, 1e30),
                 300: (nan, nan, nan), len(h) - 1: (-inf, 3e38, 1)}.items():
        h[r, :3] = v
    return h


def icp_point_inputs(small_world):
    """dict(map [20 000, 3] float32, scan [n, 3] float32, poses {name: [7]}): scan2k, 64 extra points 30–1000 m outside the map, and a
    copy of the scan's first 400 points with the hostile rows."""
    m = np.ascontiguousarray(np.asarray(small_world["map"], dtype=np.float32)[:20000, :3])
    s = np.ascontiguousarray(np.asarray(small_world["scan2k"], dtype=np.float32)[:, :3])
    rng = np.random.RandomState(20)
    ang, dist = rng.uniform(0, 2 * np.pi, 64), np.exp(rng.uniform(np.log(30.0), np.log(1000.0), 64))
    far = np.c_[(58.0 + dist) * np.cos(ang), (58.0 + dist) * np.sin(ang), rng.uniform(-5.0, 5.0, 64)].astype(np.float32)  # the map's box ends within 57 m of the sensor
    off = np.array(small_world["true_pose"], dtype=np.float64)
    off[4:] += [0.55, -0.4, 0.15]  # 0.7 m
    assert abs(np.linalg.norm(off[4:] - small_world["true_pose"][4:]) - 0.7) < 0.01
    return dict(map=m, scan=np.concatenate([s, far, hostile(s[:400])]), n_plain=len(s), n_far=64,
                poses=dict(true_pose=np.asarray(small_world["true_pose"], dtype=np.float64), init_pose=np.asarray(small_world["init_pose"], dtype=np.float64), off_0p7m=off))


def icp_point_ref(locref, inp, pose):
    """(finite [n] bool, d2 [n] float32 (NaN where not finite)) of the header's definition: q = float32(T·p) with the oracle's transform."""
    p = inp["scan"]
    fin = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        q = locref.transform_points(pose, p[fin].astype(np.float64)).astype(np.float32)
    d2 = np.full(len(p), np.nan, np.float32)
    d2[fin] = brute_d2(q, inp["map"])
    return fin, d2


def gate_of(max_range):
    """float32(max_range · max_range), the product formed in double (gn_driver.hip)."""
    return np.float32(float(max_range) * float(max_range))


# ------------------------------------------------------------------------------------------------ 2. the exact world
Q = 16       # lengths are integers in units of 1/16 m
Q2 = Q * Q   # squared distances in units of 2^-8 m²

# rotation quaternions (x, y, z, w) whose se3_apply is exact, as signed permutations of the coordinates
ROTATIONS = {(0.0, 0.0, 0.0, 1.0): (1, 1, 1), (0.0, 0.0, 1.0, 0.0): (-1, -1, 1), (1.0, 0.0, 0.0, 0.0): (1, -1, -1)}


def _axis(count, step, lo):
    """count grid values lo, lo + step, … in units of 1/16 m."""
    return lo + step * np.arange(count, dtype=np.int64)


def exact_pose(quat, t_sixteenths):
    """([7] pose, sign [3] int, t [3] int in units of 1/16 m)."""
    quat = tuple(float(v) for v in quat)
    t = np.asarray(t_sixteenths, dtype=np.int64)
    return np.array(quat + tuple(t / float(Q)), dtype=np.float64), np.array(ROTATIONS[quat], dtype=np.int64), t


def exact_apply(pose_int, src_int):
    """The pose on integer coordinates (units of 1/16 m) in integer arithmetic."""
    _, sign, t = pose_int
    return src_int * sign[None, :] + t[None, :]


def exact_world():
    """dict(
      grid = (gx [65], gy [65], gz [3]) int64, the map's axes; map [12 675, 3] float32 their product;
      edge_grid / edge_map: every second column and row of it (a coarser product grid: the LOAM tests' edge map);
      poses = [identity, half-turn about z, half-turn about x] as exact_pose tuples, each with a translation in sixteenths;
      src_int [131 073, 3] int64, the scan in its own frame in units of 1/16 m, src float32 the same;
      at_gate / above_gate: indices into the scan of the designed points whose d² under poses[1] is 1.0 and 1.0 + 2^-8.
    ). Under every pose a scan point lies at most 2.5 m outside the slab [-16, 16]² x [-0.5, 0.5] the grid spans."""
    gx, gy, gz = _axis(65, Q // 2, -16 * Q), _axis(65, Q // 2, -16 * Q), _axis(3, Q // 2, -Q // 2)
    grid = (gx, gy, gz)
    m = _product(grid)
    edge_grid = (gx[::2], gy[::2], gz)
    poses = [exact_pose((0, 0, 0, 1), (3, -5, 2)), exact_pose((0, 0, 1, 0), (-7, 4, -3)), exact_pose((1, 0, 0, 0), (6, 1, 4))]
    rng = np.random.RandomState(77)
    n = 131073
    # sixteenths: |x|, |y| <= 18 m - 1/16 (translations stay below 1/2 m), |z| <= 2.75 m - 1/16 (translations <= 1/4 m)
    src = np.stack([rng.randint(-287, 288, n), rng.randint(-287, 288, n), rng.randint(-43, 44, n)], axis=1).astype(np.int64)
    # the designed points, in the world frame of poses[1]: 1 m (and 1 m, 1/16 m aside) above the top level, below the bottom level and
    # beside the first column, at grid positions
    ix, iy = rng.randint(0, 65, 256), rng.randint(0, 65, 256)
    w = np.stack([gx[ix], gy[iy], np.where(np.arange(256) % 2 == 0, gz[2] + Q, gz[0] - Q)], axis=1)
    side = np.arange(256) % 4 == 3
    w[side] = np.stack([np.full(side.sum(), gx[0] - Q), gy[iy[side]], gz[ix[side] % 3]], axis=1)
    aside = np.arange(256) >= 128
    w[aside, 1] += np.where(rng.randint(0, 2, aside.sum()) == 0, -1, 1)  # 1/16 m along y: d² = 1 + 2^-8
    _, sign, t = poses[1]
    designed = (w - t[None, :]) * sign[None, :]  # a half-turn is its own inverse
    at = rng.permutation(4096)[:256]  # spread over the first four rows
    src[at] = designed
    out = dict(grid=grid, map=m, edge_grid=edge_grid, edge_map=_product(edge_grid), poses=poses, src_int=src, src=(src / float(Q)).astype(np.float32),
               at_gate=np.sort(at[:128]), above_gate=np.sort(at[128:]))
    assert (out["src"].astype(np.float64) * Q == src).all()
    return out


def _product(grid):
    gx, gy, gz = grid
    x, y, z = np.meshgrid(gx, gy, gz, indexing="ij")
    m = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    rng = np.random.RandomState(5)
    return (m[rng.permutation(len(m))] / float(Q)).astype(np.float32)  # no order a builder could lean on


def exact_d2(grid, world_int):
    """int64 [n]: the squared distance (units of 2^-8 m²) of every point to the nearest point of the product grid — per axis the
    nearest grid value, by brute force over the axis."""
    d2 = np.zeros(len(world_int), dtype=np.int64)
    for a in range(3):
        g = np.asarray(grid[a], dtype=np.int64)
        best = np.empty(len(world_int), dtype=np.int64)
        for lo in range(0, len(world_int), 1 << 15):
            best[lo:lo + (1 << 15)] = np.abs(world_int[lo:lo + (1 << 15), a, None] - g[None, :]).min(axis=1)
        d2 += best * best
    return d2


def exact_d2_brute(map_f32, world_int):
    """The same over ALL map points (the map taken back to integers), for a sample: the check of exact_d2."""
    mi = np.rint(np.asarray(map_f32, dtype=np.float64) * Q).astype(np.int64)
    assert (mi / float(Q) == np.asarray(map_f32, dtype=np.float64)).all()
    out = np.empty(len(world_int), dtype=np.int64)
    for i, p in enumerate(world_int):
        d = mi - p[None, :]
        out[i] = (d * d).sum(axis=1).min()
    return out


def gate_int(max_range):
    """The largest integer d² (units of 2^-8 m²) with d² / 256 <= float32(max_range²), or None for no gate."""
    g = float(gate_of(max_range))
    return None if math.isinf(g) else math.floor(g * Q2)  # g·256 is exact: a power of two


def exact_fitness(d2_int, max_range):
    """dict(score, inliers, finite_points) and (Σ, inliers) as Python integers: Σ / inliers is formed once from exact integers."""
    gi = gate_int(max_range)
    inl = np.ones(len(d2_int), bool) if gi is None else d2_int <= gi
    total, n = int(sum(int(v) for v in d2_int[inl])), int(inl.sum())
    assert total < 1 << 53
    return dict(score=(total / Q2) / n if n else float("inf"), inliers=n, finite_points=len(d2_int)), (total, n)


def joint_fitness(parts):
    """The joint LOAM score from the classes' integer (Σ, inliers, finite points): [joint, surface, edge] dicts."""
    total, n, fin = sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts)
    return dict(score=(total / Q2) / n if n else float("inf"), inliers=n, finite_points=fin)


def host_tree_depth(api, xyz):
    """Depth of the host builder's tree of a cloud (locgpu_debug_build_tree); needs no device."""
    L = api.lib()
    L.locgpu_debug_build_tree.restype = ctypes.c_size_t
    L.locgpu_debug_build_tree.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    info = np.zeros(3, dtype=np.int64)
    L.locgpu_debug_build_tree(xyz.ctypes.data, len(xyz), None, 0, info.ctypes.data)
    return int(info[2])


def gate_neighbours(max_range, span=4096):
    """(dx_at, dx_above) float32: dx_at·dx_at rounds to exactly float32(max_range²) in float32, dx_above is the next float and its
    square rounds above it — or None when no float32 squares to the gate. A CPU loop over 2·span floats around sqrt(gate)."""
    gate = gate_of(max_range)
    x = np.float32(np.sqrt(np.float64(gate)))
    for _ in range(span):
        x = np.nextafter(x, np.float32(0))
    for _ in range(2 * span):
        nxt = np.nextafter(x, np.float32(np.inf))
        if np.float32(x * x) == gate and np.float32(nxt * nxt) > gate:
            return x, nxt
        x = nxt
    return None


def gate_world(dx_at, dx_above):
    """(map [16, 3], at [16, 3], above [16, 3]) float32 in the manner of test_point_gate_keeps_a_squared_distance_equal_to_the_threshold:
    sixteen map points 16 m apart, a scan point one axis offset away from each under the identity pose. The map coordinate on that axis
    is 0, so the offset is the scan coordinate itself and dx is exact."""
    m = np.array([(16.0 * i + 0.25, 16.0 * j + 0.5, 0.75) for i in range(4) for j in range(4)], np.float32)
    at, above = np.array(m, copy=True), np.array(m, copy=True)
    for k in range(16):
        a, sgn = k % 3, np.float32(1.0 if k % 2 else -1.0)
        m[k, a] = 0.0
        at[k, a], above[k, a] = sgn * dx_at, sgn * dx_above
    return m, at, above


# ------------------------------------------------------------------------------------------------ 3. the NDT score per point
def ndt_point_ref(table, points, pose, n_nearby, voxel_size=VOXEL, res_th=RES_TH):
    """The score of every point alone at 60 digits, from the float32 point, the FP64 pose and the table's FP64 records taken as exact:
    dict(res [n, n_nearby] float64 (nearest; NaN: voxel absent), res_mp (list of lists of mpf or None), S [n, n_nearby] the scale of the
    rounding bound |e|ᵀ|info||e| + 2·|info·e|ᵀ·(|R||p| + |t|), key_margin [n] the distance of qs / voxel_size from an integer, worst
    axis, best [n] float64 (the smallest accepted residual, +inf without one), best_mp, inlier [n] bool, gate_margin [n] (relative
    distance of the nearest found residual from res_th), which [n] (index into NEARBY of the winner, -1 without one))."""
    from mpmath import mp, mpf
    p = np.asarray(points, dtype=np.float32)[:, :3]
    n = len(p)
    out = dict(res=np.full((n, n_nearby), np.nan), S=np.full((n, n_nearby), np.nan), key_margin=np.zeros(n), best=np.full(n, np.inf),
               inlier=np.zeros(n, bool), gate_margin=np.full(n, np.inf), which=np.full(n, -1), res_mp=[], best_mp=[], pairs=0)
    with mp.workdps(60):
        q = [mpf(float(v)) for v in pose[:4]]
        t = [mpf(float(v)) for v in pose[4:]]
        x, y, z, w = q
        # v + w·2(qv × v) + qv × 2(qv × v), written out as a matrix: what se3_apply and the oracle's transform evaluate for this q
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        inv = mpf(1.0 / voxel_size)
        th = mpf(res_th)
        for i in range(n):
            v = [mpf(float(c)) for c in p[i]]
            qs = [R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2] + t[r] for r in range(3)]
            reach = [abs(R[r][0]) * abs(v[0]) + abs(R[r][1]) * abs(v[1]) + abs(R[r][2]) * abs(v[2]) + abs(t[r]) for r in range(3)]
            scaled = [c * inv for c in qs]
            key = [int(c) for c in scaled]  # int() of an mpf truncates toward zero
            out["key_margin"][i] = float(min(min(c - mp.floor(c), mp.ceil(c) - c) if c != mp.floor(c) else mpf(0) for c in scaled))
            vid = table.find(np.array(key, dtype=np.int64)[None, :] + ndt_score_ref.NEARBY[:n_nearby])
            row, best, which = [], None, -1
            for j in range(n_nearby):
                if vid[j] < 0:
                    row.append(None)
                    continue
                out["pairs"] += 1
                mu, info = table.mu[vid[j]], table.info[vid[j]]
                e = [qs[r] - mpf(float(mu[r])) for r in range(3)]
                I = [[mpf(float(info[r, c])) for c in range(3)] for r in range(3)]
                ie = [sum(I[r][c] * e[c] for c in range(3)) for r in range(3)]
                res = sum(e[r] * ie[r] for r in range(3))
                row.append(res)
                out["res"][i, j] = float(res)
                out["S"][i, j] = float(sum(abs(e[r]) * abs(I[r][c]) * abs(e[c]) for r in range(3) for c in range(3)) + 2 * sum(abs(ie[r]) * reach[r] for r in range(3)))
                out["gate_margin"][i] = min(out["gate_margin"][i], float(abs(res - th) / th))
                if not res > th and (best is None or res < best):
                    best, which = res, j
            out["res_mp"].append(row)
            out["best_mp"].append(best)
            out["which"][i] = which
            if best is not None:
                out["best"][i], out["inlier"][i] = float(best), True
    return out


def err_in_units(got, ref_mp, S):
    """|got − ref| / (u·S) with the difference formed at 60 digits."""
    from mpmath import mp, mpf
    with mp.workdps(60):
        return float(abs(mpf(float(got)) - ref_mp) / (mpf(U) * mpf(float(S))))


def classify(res, res_th=RES_TH):
    """From residuals [n, k] (NaN: absent): (best [n], which [n] or -1, not_centre [n]: the smallest accepted residual is not the centre
    voxel's while the centre's is accepted too, rescued [n]: the centre voxel is refused or absent and a neighbour accepted, none [n])."""
    with np.errstate(invalid="ignore"):
        accept = ~(np.isnan(res) | (res > res_th))
    val = np.where(accept, res, np.inf)
    which = np.where(accept.any(axis=1), val.argmin(axis=1), -1)
    return val.min(axis=1), which, accept[:, 0] & (which > 0), ~accept[:, 0] & (which > 0), which < 0


def ndt_point_inputs(locref, table, small_world, per_pose=(70, 40, 30, 60)):
    """The compared points of the per-point NDT tests, chosen with the numpy restatement on `table` (the oracle's on the CPU, the GPU's
    own dump on the GPU; in both cases of the small world's WHOLE map: its first 20 000 points fill few voxels) from scan2k at true_pose and init_pose with seven probed voxels: per pose up to 70 points whose smallest
    accepted residual is not the centre voxel's, 40 whose centre voxel is refused or absent while a neighbour is accepted, 30 without an
    accepted voxel and 60 others, in scan order. [(name, pose, points [n, 3] float32)]. About 1 600 point–voxel pairs for the mpmath
    restatement with NEARBY6, and the same points again with CENTER."""
    s = np.ascontiguousarray(np.asarray(small_world["scan2k"], dtype=np.float32)[:, :3])
    out = []
    for name in ("true_pose", "init_pose"):
        pose = np.asarray(small_world[name], dtype=np.float64)
        res = ndt_score_ref.residuals(locref, table, s, pose, VOXEL, 7)
        _, which, not_centre, rescued, none = classify(res)
        rest = ~(not_centre | rescued | none)
        pick = np.concatenate([np.flatnonzero(c)[:k] for c, k in zip((not_centre, rescued, none, rest), per_pose)])
        out.append((name, pose, s[np.sort(pick)]))
    return out


def ndt_gate_case(table, v, voxel_size=VOXEL):
    """(translation [3] FP64, threshold) of voxel v of the table, or None when the voxel does not serve (see ndt_gate_cases)."""
    mu, info = table.mu[v], table.info[v]
    frac = mu[0] / voxel_size - np.floor(mu[0] / voxel_size)
    if not ((mu > voxel_size).all() and np.isfinite(info).all() and info[0, 0] > 0 and 0.2 < frac < 0.8):
        return None
    qx = mu[0] + (0.125 if frac < 0.5 else -0.125) * voxel_size
    e = qx - mu[0]
    assert float(np.float64(qx) - np.float64(e)) == mu[0]  # the difference is exact
    return np.array([qx, mu[1], mu[2]]), float((e * info[0, 0]) * e)


def ndt_gate_cases(table, count=8, voxel_size=VOXEL):
    """[(translation [3] FP64, threshold, packed key of the voxel)]: the point (0, 0, 0) under the identity rotation and this translation
    lands at qs = mu + (δ, 0, 0) of a voxel, δ = ±1/8 (up to the rounding of mu.x + δ; qs.x − mu.x is then exact), inside the voxel's
    cell. With one non-zero component of e every association of eᵀ·info·e gives res = fl(fl(δ·info[0][0])·δ): the other products are
    zeros. That value is the threshold: the residual EQUALS res_outlier_th."""
    out = []
    for v in range(len(table.packed)):
        c = ndt_gate_case(table, v, voxel_size)
        if c is not None:
            out.append(c + (int(table.packed[v]),))
        if len(out) == count:
            break
    return out


def tiled(scan, n):
    """The scan repeated to n points."""
    s = np.ascontiguousarray(np.asarray(scan, dtype=np.float32)[:, :3])
    return np.ascontiguousarray(np.tile(s, (n // len(s) + 1, 1))[:n])
