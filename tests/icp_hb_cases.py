"""Inputs shared by tests/test_icp_hb_ref.py (CPU) and tests/test_gpu_icp_hb.py (GPU): the two input sets of the per-point ICP tests,
the exclusions, the conditions of the input and the recorded units.

Input sets. (1) The small-world sample: 512 points of scan10k against the small world's map, at true_pose and at init_pose, default
options (approximate search, α = 0.1). (2) The designed map: clusters of five points at least 6 m apart, so that a query near a
cluster's centre has exactly that cluster as its five nearest neighbours under either search mode — neighbourhoods by design, PER_KIND
of each of KINDS, two queries per cluster, evaluated with the exact search.

Exclusions, each decided from the restatement alone (excluded()): a gated quantity within GATE_REL (relative) of its gate, κ > KAPPA_MAX,
and rank-deficient neighbourhoods (whose vector is a convention shared with the checker: they are compared with the oracle only, by
the aggregate bar).

The measure is error / (u·κ) (icp_hb_ref.in_units): the error of a fitted singular vector grows with κ, which spans 70 … 1.5e7 over
these inputs, so no absolute bar can serve them all; a backward-stable fit promises O(1) in this measure whatever the input."""
import numpy as np

import icp_hb_ref as ref

P2P, P2LINE, P2PLANE, MAPPLANE = ref.P2P, ref.P2LINE, ref.P2PLANE, ref.MAPPLANE
ORACLE_METHODS = (P2P, P2LINE, P2PLANE)
NAMES = {P2P: "P2P", P2LINE: "P2Line", P2PLANE: "P2Plane", MAPPLANE: "map-plane"}
K_OF = {P2P: 1, P2LINE: 5, P2PLANE: 5, MAPPLANE: 1}

GATE_REL = 1e-9       # a gated quantity this close (relative) to its gate may fall either side of it
KAPPA_MAX = 1e8       # beyond it u·κ passes 1e-8, the aggregate bar: nothing is left to assert per point
MAX_EXCLUDED = 0.01   # share of the small-world sample that may be excluded
MIN_ACCEPTED = 256    # accepted points per method and pose of the small-world sample
BAR_FACTOR = 8.0      # the project's factor (ndt_hb_cases.BAR_FACTOR)

# The per-point unit: the ORACLE's own worst error / (u·κ) against the restatement over both input sets, per method and quantity, measured
# and printed by test_icp_hb_ref.py::test_per_point_unit_of_the_oracle (H, B) and ::test_oracle_fits_against_the_exact_vectors (n4, the
# line direction), recorded here rounded up to two digits and never below 1 — a backward-stable fit promises O(1) in this measure, and a
# lucky oracle must not set a bar below that. The test checks that these figures are not below what it measures. The map-plane
# mode's oracle is map_plane_ref.hb (FP64 numpy over oracle pieces) fed the oracle's table rows; κ = 1: the table is data there.
UNIT = {
    P2P: dict(H=4.1, B=420.0),      # measured 4.04, 413 (B: e = p − qs cancels 500 m down to centimetres on the far patches)
    P2LINE: dict(H=11.0, B=320.0),  # measured 10.8, 316
    P2PLANE: dict(H=27.0, B=1.0),   # measured 26.9, 0.168
    MAPPLANE: dict(H=85.0, B=52.0),  # measured 84.5, 51.0 (map_plane_ref.hb, the FP64 numpy restatement of the mode, on the oracle's rows)
    "n4": 1.0,                      # measured 0.359 (0.068 on the small world)
    "line_d": 3.9,                  # measured 3.83
}

KINDS = ("noise_2e-2", "noise_1e-3", "noise_1e-5", "noise_2e-8", "through_origin", "collinear_1e-2", "collinear_1e-3", "far_300_500m",
         "coplanar_exact", "collinear_exact")
EXACT_KINDS = ("coplanar_exact", "collinear_exact")  # the only kinds in which a neighbourhood may be excluded
PER_KIND = 24
DESIGNED_POSE = np.array([0.02, -0.03, 0.17, 0.0, 1.5, -2.5, 0.25])
DESIGNED_POSE[3] = np.sqrt(1.0 - (DESIGNED_POSE[:3] ** 2).sum())


def sample_points(small_world):
    """The 512 points of scan10k, spread over its rings."""
    return np.ascontiguousarray(small_world["scan10k"][::19][:512])


def neighbours(locref, tree, scan, pose, method, approximate=True, alpha=0.1):
    """The oracle tree's answer to the oracle's own query: the FP64-transformed point cast to float (locref.cpp CastF). [n, k] int32."""
    s = np.ascontiguousarray(np.asarray(scan, dtype=np.float32)[:, :3])
    qs = locref.transform_points(pose, s.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        return tree.knn(qs.astype(np.float32), k=K_OF[method], approximate=approximate, alpha=alpha)


def _frame(rng):
    """A random orthonormal frame (rows)."""
    q, _ = np.linalg.qr(rng.randn(3, 3))
    return q.T


def designed_map(seed=2024):
    """(map float32 [5·n, 3], kind [n] index into KINDS, cluster c holding rows 5c … 5c + 4). Plane patches of radius 0.3 m with
    normal noise 2e-2, 1e-3 m (any orientation) and 1e-5, 2e-8 m (horizontal, z a few cm: float32 keeps that noise there); planes
    through the origin; near-collinear patches with lateral spread 1e-2 and 1e-3 m; patches 300–500 m from the origin; exactly coplanar
    clusters (z constant, x and y on a float grid); exactly collinear clusters (equal steps on a float grid)."""
    rng = np.random.RandomState(seed)
    pts, kinds = [], []
    near_kinds = [k for k in KINDS if k != "far_300_500m"]
    cells = [(ix, iy) for iy in range(14) for ix in range(16)]
    order = rng.permutation(len(cells))
    at = 0
    for kind in KINDS:
        for j in range(PER_KIND):
            if kind == "far_300_500m":
                a, r = 2 * np.pi * (j + 0.3) / PER_KIND, rng.uniform(300.0, 500.0)
                c = np.array([r * np.cos(a), r * np.sin(a), rng.uniform(-3.0, 3.0)])
            else:
                ix, iy = cells[order[at]]
                at += 1
                c = np.array([(ix - 7.5) * 8.0 + rng.uniform(-0.5, 0.5), (iy - 6.5) * 8.0 + rng.uniform(-0.5, 0.5), rng.uniform(-3.0, 3.0)])
            f = _frame(rng)
            if kind.startswith("noise_") or kind in ("through_origin", "far_300_500m"):
                noise = {"noise_2e-2": 2e-2, "noise_1e-3": 1e-3, "noise_1e-5": 1e-5, "noise_2e-8": 2e-8, "through_origin": 1e-3, "far_300_500m": 1e-2}[kind]
                if kind in ("noise_1e-5", "noise_2e-8"):
                    f = np.eye(3)
                    c[2] = rng.uniform(0.03, 0.06)
                if kind == "through_origin":  # the normal f[2] orthogonal to the centre: the plane holds the origin
                    n = np.cross(c, rng.randn(3))
                    n /= np.linalg.norm(n)
                    u = np.cross(n, c / np.linalg.norm(c))
                    f = np.stack([u, np.cross(n, u), n])
                ang, rad = rng.uniform(0, 2 * np.pi, 5), 0.3 * np.sqrt(rng.uniform(0.05, 1.0, 5))
                p = c + np.outer(rad * np.cos(ang), f[0]) + np.outer(rad * np.sin(ang), f[1]) + np.outer(noise * rng.randn(5), f[2])
            elif kind in ("collinear_1e-2", "collinear_1e-3"):
                spread = 1e-2 if kind == "collinear_1e-2" else 1e-3
                along = np.array([-0.3, -0.15, 0.0, 0.15, 0.3]) + rng.uniform(-0.05, 0.05, 5)
                p = c + np.outer(along, f[0]) + np.outer(spread * rng.randn(5), f[1]) + np.outer(spread * rng.randn(5), f[2])
            elif kind == "coplanar_exact":
                c = np.round(c * 64.0) / 64.0
                p = np.tile(c, (5, 1))
                while True:
                    off = rng.randint(-76, 77, (5, 2)) / 256.0
                    if len({tuple(o) for o in off}) == 5 and abs(np.linalg.det(np.c_[off[:3], np.ones(3)])) > 1e-3:
                        break
                p[:, :2] += off
            else:  # collinear_exact
                c = np.round(c * 64.0) / 64.0
                while True:
                    d = rng.randint(-3, 4, 3)
                    if d.any():
                        break
                p = c + np.outer(np.arange(-2, 3), d / 32.0)
            pts.append(p)
            kinds.append(KINDS.index(kind))
    assert at <= len(cells) and len(near_kinds) * PER_KIND == at
    return np.concatenate(pts).astype(np.float32), np.array(kinds)


def designed_scan(m, pose=DESIGNED_POSE, seed=7):
    """(scan float32 [2·n, 3], cluster [2·n]): two source points per cluster which `pose` carries to within 5 cm of the cluster's
    centroid — inside every gate of the default options."""
    rng = np.random.RandomState(seed)
    n = len(m) // 5
    cen = m.astype(np.float64).reshape(n, 5, 3).mean(axis=1)
    cluster = np.repeat(np.arange(n), 2)
    off = rng.randn(2 * n, 3)
    off *= (0.05 * rng.uniform(0.2, 1.0, 2 * n) / np.linalg.norm(off, axis=1))[:, None]
    w = cen[cluster] + off
    R = np.array([[float(v) for v in row] for row in ref.rotation(pose)])
    return ((w - pose[4:]) @ R).astype(np.float32), cluster  # Rᵀ·(w − t)


def input_sets(locref, small_world):
    """name → dict(map, tree (the oracle's), scan, pose, approximate, kind ([n] index into KINDS, or None)): the small-world sample at
    its two poses and the designed map."""
    pts = sample_points(small_world)
    small = locref.KdTree(small_world["map"])
    dm, kind = designed_map()
    ds, cluster = designed_scan(dm)
    return {
        "true_pose": dict(map=small_world["map"], tree=small, scan=pts, pose=small_world["true_pose"], approximate=True, kind=None),
        "init_pose": dict(map=small_world["map"], tree=small, scan=pts, pose=small_world["init_pose"], approximate=True, kind=None),
        "designed": dict(map=dm, tree=locref.KdTree(dm), scan=ds, pose=DESIGNED_POSE, approximate=False, kind=kind[cluster]),
    }


def restate(locref, inp, method, planes=None):
    """ref.per_point of the input set `inp` with the oracle tree's neighbour lists."""
    nn = neighbours(locref, inp["tree"], inp["scan"], inp["pose"], method, approximate=inp["approximate"])
    pp = ref.per_point(method, inp["map"], nn, inp["scan"], inp["pose"], planes=planes)
    pp["nn"] = nn
    return pp


def exact_neighbourhoods(tree, map_xyz, rows):
    """[len(rows), 5] the exact 5-NN (the oracle tree's) of the map points `rows`, themselves included: what the plane table fits."""
    m = np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, :3])
    return tree.knn(m[rows], k=5, approximate=False)


def oracle_plane_rows(locref, tree, map_xyz, rows):
    """(n4 [n_map, 4], valid [n_map]) of the oracle's plane table (map_plane_ref.plane_table), only the rows `rows` filled in."""
    m = np.ascontiguousarray(np.asarray(map_xyz, dtype=np.float32)[:, :3])
    n4, valid = np.zeros((len(m), 4)), np.zeros(len(m), dtype=bool)
    rows = np.unique(rows)
    for i, nn in zip(rows, exact_neighbourhoods(tree, m, rows)):
        valid[i], n4[i] = locref.fit_plane(m[nn].astype(np.float64))
    return n4, valid


def excluded(pp):
    """Points [n] bool that are not compared per point (see the module's docstring), from the restatement alone."""
    with np.errstate(invalid="ignore"):
        return ref.near_gate(pp, GATE_REL) | ~(pp["kappa"] <= KAPPA_MAX) | pp["rank_deficient"]


def assert_per_point(tag, method, hb, pp, inp):
    """The per-point assertions on hb [n, 44] — row i the 44-double row (H 36 row-major, B 6, effective_num, ok; gn_update's hb_out
    in icp_fit.hip) of a scan holding point i alone — against the restatement pp of the input set inp. On the non-excluded points:
    finite rows, H == Hᵀ, effective_num == fitted, the accepted witness (H.any(); effective_num for P2P), error / (u·κ) <= 8 × UNIT for
    H and B. `ok` is not compared: a one-point H is singular. Prints worst observed next to bar and unit, per kind; a point above the
    bar is printed with its coordinates, its neighbours and κ first. Returns the worst (H, B) in units."""
    H, B, eff = hb[:, :36].reshape(-1, 6, 6), hb[:, 36:42], hb[:, 42]
    keep = ~excluded(pp)
    assert np.isfinite(hb[keep]).all()
    assert np.array_equal(H[keep], H[keep].transpose(0, 2, 1))
    fitted_differs = np.flatnonzero(keep & (eff != pp["fitted"]))
    witness = eff > 0 if method == P2P else H.reshape(len(H), -1).any(axis=1)
    accepted_differs = np.flatnonzero(keep & (witness != pp["accepted"]))
    print("%s %s: %d compared, %d excluded; effective_num differs on %d, the accepted witness on %d"
          % (tag, NAMES[method], keep.sum(), (~keep).sum(), len(fitted_differs), len(accepted_differs)))
    assert len(fitted_differs) == 0 and len(accepted_differs) == 0, (fitted_differs[:8], accepted_differs[:8])
    uh, ub = units(H, B, pp)
    bar_h, bar_b = BAR_FACTOR * UNIT[method]["H"], BAR_FACTOR * UNIT[method]["B"]
    groups = [("all", keep)] if inp["kind"] is None else [(KINDS[k], keep & (inp["kind"] == k)) for k in range(len(KINDS))]
    for name, sel in groups:
        if sel.any():
            print("    %-16s kappa %.3g … %.3g  worst error / (u·kappa): H %.3g (bar %.3g = 8 x %.3g), B %.3g (bar %.3g = 8 x %.3g)"
                  % (name, pp["kappa"][sel].min(), pp["kappa"][sel].max(), uh[sel].max(), bar_h, UNIT[method]["H"], ub[sel].max(), bar_b, UNIT[method]["B"]))
    m = np.asarray(inp["map"], dtype=np.float32)
    for i in np.flatnonzero(keep & ((uh > bar_h) | (ub > bar_b)))[:8]:
        print("    ABOVE THE BAR: point %d = %s, kappa %.6g, H %.3g units, B %.3g units, neighbours %s:\n%s"
              % (i, inp["scan"][i, :3].tolist(), pp["kappa"][i], uh[i], ub[i], pp["nn"][i].tolist(), m[pp["nn"][i], :3].tolist()))
    assert uh[keep].max() <= bar_h and ub[keep].max() <= bar_b, (tag, method, uh[keep].max(), ub[keep].max())
    return uh[keep].max(), ub[keep].max()


def one_point_rows(ctx, scan, pose, opts):
    """icp_hb_batch of a batch of len(scan) one-point scans, all at `pose`: a per-point dump of the accumulate kernel. [n, 44]."""
    b = ctx.batch([scan[i:i + 1] for i in range(len(scan))])
    try:
        return ctx.icp_hb_batch(b, np.stack([pose] * len(scan)), opts)
    finally:
        b.close()


def units(Hg, Bg, pp):
    """(H, B) errors of the rows Hg [n, 6, 6], Bg [n, 6] in units of u·κ, float64 [n]."""
    eh, eb = ref.point_errors(Hg, Bg, pp)
    return ref.in_units(eh, pp["kappa"]), ref.in_units(eb, pp["kappa"])
