"""The designed inputs of tests/test_gpu_grid_lists.py, shared with tests/test_grid_route_ref.py (which shows on the CPU, with
grid_route_ref.ladder() in place of the library's grid, that each input reaches the path of the grid search it is named for).

A case is a dict: map [n, 3] float32, scan [m, 3] float32 (scan frame), pose [7] (quaternion xyzw + t), cap (the largest share of the
queries that may go to the tree, or None) and `want`, the queries in the map frame as designed (float64; what the kernels see is the
float32 of the pose applied to the float32 scan). Everything is seeded. Volumetric maps are avoided on purpose: at the build's ≈4
leaves per occupied cell an 8×8×8-cell block of a filled volume holds ≈1 900 leaves, more than the 1 024 the tile kernel stages, so
such a map tests the tree fallback (grid_route_ref.route: no_fit), not the tile kernel.
"""
import numpy as np

import grid_route_ref as R

IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
SHIFT = np.array([0.0, 0.0, 0.0, 1.0, 0.05, -0.03, 0.02])  # translation only
_q = np.array([0.01, -0.02, 0.03, 1.0])
TILT = np.concatenate([_q / np.linalg.norm(_q), [0.05, -0.03, 0.02]])


def rot(pose):
    x, y, z, w = pose[:4]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scan_for(want, pose):
    """The float32 scan whose points land on `want` (map frame) under `pose`, up to float32 rounding."""
    if np.array_equal(pose, IDENT):
        return np.asarray(want, dtype=np.float32)
    return ((np.asarray(want, dtype=np.float64) - pose[4:]) @ rot(pose)).astype(np.float32)


def inside(want, m, margin=1e-3):
    """`want` clipped into the map's bounding box, `margin` away from its faces where the box is thicker than that."""
    lo, hi = m.min(axis=0).astype(np.float64), m.max(axis=0).astype(np.float64)
    thin = (hi - lo) <= 4 * margin
    mid = 0.5 * (lo + hi)
    return np.where(thin, np.clip(want, mid, mid), np.clip(want, lo + margin, hi - margin))


def case(name, m, want, pose, cap, **kw):
    m = np.ascontiguousarray(m, dtype=np.float32)
    return dict(name=name, map=m, want=np.asarray(want, dtype=np.float64), scan=scan_for(want, pose), pose=pose, cap=cap, **kw)


# ---- maps
def _surface(rng, n):
    k = rng.randint(0, 4, n)
    u, v = rng.uniform(-9.5, 9.5, n), rng.uniform(0.2, 3.8, n)
    w = rng.uniform(-9.5, 9.5, n)
    g = np.stack([u, w, np.zeros(n)], 1)
    wx = np.stack([np.full(n, 10.0), u, v], 1)
    wy = np.stack([u, np.full(n, 10.0), v], 1)
    return np.where((k < 2)[:, None], g, np.where((k == 2)[:, None], wx, wy))


def room_map():
    """A ground patch and two walls with 1 cm noise, 6 000 points: the body of test_gpu_plane_dedup.py's map (same seed and draw)."""
    rng = np.random.RandomState(11)
    return (_surface(rng, 6000) + rng.normal(0.0, 0.01, (6000, 3))).astype(np.float32)


def sheet_map(seed=21, n=4096, half=20.0, thick=0.005):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), rng.uniform(-thick / 2, thick / 2, n)], 1).astype(np.float32)


def _near(rng, m, n, sigma, z_sigma=None):
    """n points: map points drawn with replacement plus noise (z_sigma for the third axis when it differs), inside the bounding box."""
    s = np.array([sigma, sigma, sigma if z_sigma is None else z_sigma])
    return inside(m[rng.randint(0, len(m), n)].astype(np.float64) + rng.normal(0.0, 1.0, (n, 3)) * s, m)


# ---- cases with one scan
def room():
    m = room_map()
    return case("room", m, _near(np.random.RandomState(31), m, 4000, 0.03), TILT, 0.02)


def sheet():
    m = sheet_map()
    return case("sheet", m, _near(np.random.RandomState(32), m, 3000, 0.3, 0.001), TILT, 0.02)


def line():
    rng = np.random.RandomState(33)
    m = np.zeros((4096, 3), np.float32)
    m[:, 0] = rng.uniform(0.0, 400.0, 4096)
    want = np.zeros((3000, 3))
    want[:, 0] = np.clip(rng.uniform(0.0, 400.0, 3000), float(m[:, 0].min()) + 1e-3, float(m[:, 0].max()) - 1e-3)
    return case("line", m, want, np.array([0.0, 0.0, 0.0, 1.0, 0.05, 0.0, 0.0]), 0.02)


def wide():
    """32 768 points on a 110 m square; 2 048 queries dealt round-robin over the occupied tiles (of the grid ladder() restates), so
    that every 256-query block of the bin kernels merges ≥ 200 distinct keys in its LDS hash."""
    m = sheet_map(seed=41, n=32768, half=55.0)
    g = R.ladder(m)
    rng = np.random.RandomState(42)
    tiles = rng.permutation(g["tile_lin"])
    _, _, lin = R.query_cells(g, m)
    by_tile = {t: np.nonzero(lin == t)[0] for t in tiles}
    pick = np.array([rng.choice(by_tile[tiles[i % len(tiles)]]) for i in range(2048)])
    want = inside(m[pick].astype(np.float64) + rng.normal(0.0, 1.0, (2048, 3)) * [0.02, 0.02, 0.0005], m)
    return case("wide", m, want, TILT, 0.02)


HOT_RUNS = [1, 255, 256, 257, 700]
OFFSET = np.array([1e5, -3e4, 50.0])


def hot_tiles():
    """Room map; runs of 1, 255, 256, 257 and 700 queries inside one tile each (five tiles, chosen among those with the most
    leaves, of the grid ladder() restates) and 1 500 spread ones, shuffled: after the sort by tile the long runs start inside a
    256-query range and cross one or two of its boundaries, so the tile's block is staged again in the next range."""
    m = room_map()
    g = R.ladder(m)
    rng = np.random.RandomState(51)
    _, _, lin = R.query_cells(g, m)
    tiles, counts = np.unique(lin, return_counts=True)
    hot = tiles[np.argsort(-counts, kind="stable")[:len(HOT_RUNS)]]
    td, cell, o = g["tdims"], float(g["cell"]), g["origin"].astype(np.float64)
    parts = []
    for t, n in zip(hot, HOT_RUNS):
        txyz = np.array([t % td[0], (t // td[0]) % td[1], t // (td[0] * td[1])], dtype=np.float64)
        lo, hi = o + 4 * txyz * cell + 0.01, o + 4 * (txyz + 1) * cell - 0.01
        idx = np.nonzero(lin == t)[0]
        p = m[idx[rng.randint(0, len(idx), n)]].astype(np.float64) + rng.normal(0.0, 0.02, (n, 3))
        parts.append(inside(np.clip(p, lo, hi), m))
    parts.append(_near(rng, m, 1500, 0.03))
    want = np.concatenate(parts)
    return case("hot_tiles", m, want[rng.permutation(len(want))], TILT, 0.02, hot=hot)


def sparse_half(n_thin=296):
    """3 800 points on one half of the sheet set the cell edge; the n_thin = 296 on the other half leave most cells there empty, so k = 5
    needs the 5×5×5 shell."""
    rng = np.random.RandomState(61)
    dense = np.stack([rng.uniform(-20, 0, 3800), rng.uniform(-20, 20, 3800), rng.uniform(-0.0025, 0.0025, 3800)], 1)
    thin = np.stack([rng.uniform(0, 20, n_thin), rng.uniform(-20, 20, n_thin), rng.uniform(-0.0025, 0.0025, n_thin)], 1)
    m = np.concatenate([dense, thin]).astype(np.float32)
    want = _near(rng, thin.astype(np.float32), 2000, 0.8, 0.001)  # around the sparse half's own points: few of them stay open after ring 2
    want[:, 0] = np.maximum(want[:, 0], 0.3)
    want = inside(want, m)
    return case("sparse_half", m, want, TILT, 0.15, ring2_share=0.5)


def _tilt45(p):
    """Rotation by 45° about x: the sheet's plane then cuts the grid diagonally, through the cells with dy = dz."""
    r = np.sqrt(0.5)
    return np.stack([p[:, 0], r * (p[:, 1] - p[:, 2]), r * (p[:, 1] + p[:, 2])], 1)


def sparse_tilted():
    """sparse_half turned by 45° about x: a 3-D grid in which the 5×5×5 shell's rows with |dy| = |dz| = 2 — its first and its last row
    among them — hold the leaves that k = 5 needs. On the flat sheet every row of the shell with dz ≠ 0 is empty. (800 points on the
    sparse half: the diagonal cut leaves fewer leaves per cell.)"""
    c = sparse_half(n_thin=800)
    m = np.unique(_tilt45(c["map"].astype(np.float64)).astype(np.float32), axis=0)
    m = m[np.random.RandomState(62).permutation(len(m))]
    return case("sparse_tilted", m, inside(_tilt45(c["want"]), m), TILT, 0.15, ring2_share=0.3)


def sparse_offset():
    """sparse_half moved to (1e5, −3e4, 50): slack (0.19 m here, set by max_abs) decides for some of the queries whether ring 2
    settles them or the tree has to."""
    c = sparse_half()
    m = np.unique((c["map"].astype(np.float64) + OFFSET).astype(np.float32), axis=0)
    m = m[np.random.RandomState(63).permutation(len(m))]
    return case("sparse_offset", m, inside(c["want"] + OFFSET, m, margin=0.02), np.concatenate([TILT[:4], OFFSET + [0.05, -0.03, 0.0]]), 0.15)


def clump():
    """The sheet plus 1 500 distinct points inside 8 mm: the blocks that hold the clump exceed the stage (fits == false), their
    neighbours are staged as usual."""
    rng = np.random.RandomState(71)
    s = sheet_map()
    c = np.array([3.0, -2.0, 0.0]) + rng.uniform(-0.004, 0.004, (1500, 3)) * [1, 1, 0.5]
    m = np.unique(np.concatenate([s, c.astype(np.float32)]), axis=0)
    m = m[rng.permutation(len(m))]
    return case("clump", m, _near(rng, s, 3000, 0.3, 0.001), TILT, 0.15, no_fit_share=0.01)


def offset():
    """The sheet moved to (1e5, −3e4, 50): float32 resolves 8 mm in x there; slack is set by max_abs. The pose carries the offset,
    the scan lies near the origin."""
    m = (sheet_map().astype(np.float64) + OFFSET).astype(np.float32)
    m = np.unique(m, axis=0)
    m = m[np.random.RandomState(81).permutation(len(m))]
    want = _near(np.random.RandomState(82), m, 3000, 0.3, 0.001)
    want = inside(want, m, margin=0.02)
    return case("offset", m, want, np.concatenate([TILT[:4], OFFSET + [0.05, -0.03, 0.0]]), 0.05)


def _tie_queries(rng, lat, step, flat):
    d = 2 if flat else 3
    centre = lat[rng.randint(0, len(lat), 600)].astype(np.float64)
    centre[:, :d] += step / 2  # cell centres: 2^d equal distances
    half = lat[rng.randint(0, len(lat), 600)].astype(np.float64)
    half[np.arange(600), rng.randint(0, d, 600)] += step / 2  # halfway between two lattice points, exact in float32
    noisy = lat[rng.randint(0, len(lat), 800)].astype(np.float64)
    noisy[:, :d] += rng.normal(0.0, 0.05, (800, d))
    return inside(np.concatenate([centre, half, noisy]), lat, margin=0.0)


def ties():
    """A 16³ lattice of 0.5 m. (A filled volume: route() says how much of it the tile kernel sees at all — see ties_flat.)"""
    g = np.arange(16, dtype=np.float64) * 0.5
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return case("ties", lat, _tie_queries(np.random.RandomState(91), lat, 0.5, False), IDENT, None, tie_bound=True)


def ties_flat():
    """A 64×64 lattice of 0.5 m in the plane z = 0: the same three kinds of queries, on a map whose blocks fit the stage, so the ties
    are met by TopK::offer and finish() and not by the no_fit early-out."""
    g = np.arange(64, dtype=np.float64) * 0.5
    lat = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return case("ties_flat", lat, _tie_queries(np.random.RandomState(92), lat, 0.5, True), IDENT, None, tie_bound=True)


def room_edges():
    """Room map, identity pose: queries within one cell outside each face of the grid, 1 km and 1e17 away, and on the minimum and the
    maximum corner of the bounding box."""
    m = room_map()
    g = R.ladder(m)
    rng = np.random.RandomState(101)
    lo, cell = g["origin"].astype(np.float64), float(g["cell"])
    top = lo + g["dims"] * cell  # the grid's upper faces (≥ the bounding box's)
    parts = []
    for a in range(3):
        for side in (0, 1):
            p = _near(rng, m, 40, 0.03)
            p[:, a] = lo[a] - rng.uniform(0.001, 0.999, 40) * cell if side == 0 else top[a] + rng.uniform(0.001, 0.999, 40) * cell
            parts.append(p)
    far = _near(rng, m, 12, 0.03)
    far[np.arange(6), rng.randint(0, 3, 6)] += 1000.0
    far[6:9, 0] = 1e17
    far[9:, 1] = -1e17
    parts.append(far)
    parts.append(np.stack([m.min(axis=0), m.max(axis=0)]).astype(np.float64))
    parts.append(_near(rng, m, 100, 0.03))
    return case("room_edges", m, np.concatenate(parts), IDENT, None, n_outside_min=6 * 40 + 12)


SINGLE = [room, sheet, line, wide, hot_tiles, sparse_half, sparse_tilted, sparse_offset, clump, offset, ties, ties_flat, room_edges]


def tiny_targets():
    """[(name, map, queries)] — targets of 1, 4, 5, 6 and 12 leaves and one whose points are all equal; queries around them, identity pose.
    Axes of 1 to 3 cells: settle_top's `cx − R > 0` and `cx + R < nx − 1` at R = 1 and 2."""
    rng = np.random.RandomState(111)
    pts = rng.uniform(-1.0, 1.0, (6, 3)).astype(np.float32)
    q = np.concatenate([rng.uniform(-1.0, 1.0, (60, 3)), rng.uniform(-3.0, 3.0, (40, 3)), pts.astype(np.float64)]).astype(np.float32)
    out = [("leaves%d" % n, pts[:n].copy(), q) for n in (1, 4, 5, 6)]
    out.append(("all_equal", np.repeat(pts[:1], 7, axis=0), q))
    # twelve points a metre apart along x: the ladder stops at three cells on that axis, one on the others
    row = np.zeros((12, 3), np.float32)
    row[:, 0] = np.arange(12)
    row[:, 1:] = rng.uniform(0.0, 0.01, (12, 2))
    qr = np.stack([rng.uniform(0.0, 11.0, 120), rng.uniform(0.0, 0.01, 120), rng.uniform(0.0, 0.01, 120)], 1).astype(np.float32)
    out.append(("row12", row, qr))
    return out


# ---- batches on the room map
def batch_poses(n, seed=121):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        q = np.concatenate([rng.normal(0.0, 0.01, 3), [1.0]])
        out.append(np.concatenate([q / np.linalg.norm(q), rng.normal(0.0, 0.05, 3)]))
    return np.stack(out)


BATCH_COUNTS = [0, 1, 255, 256, 257, 2000]
COPIES = 270  # × 2 000 points = 2 110 ranges of 256 for 2 048 waves: the grid-stride loop over ranges runs


def ragged_batch():
    """(map, scans, poses): counts 0, 1, 255, 256, 257 and 2 000 under six poses."""
    m = room_map()
    rng = np.random.RandomState(122)
    poses = batch_poses(len(BATCH_COUNTS))
    scans = [scan_for(_near(rng, m, n, 0.03), p) if n else np.zeros((0, 3), np.float32) for n, p in zip(BATCH_COUNTS, poses)]
    return m, scans, poses


def shared_pair():
    """(map, scan, two poses): one resident scan read by two entries of a shared-source batch. The scan keeps half a metre from the
    faces of the bounding box, so that it stays inside under both poses."""
    m = room_map()
    poses = batch_poses(2, seed=123)
    want = inside(_near(np.random.RandomState(124), m, 2000, 0.03), m, margin=0.5)
    return m, scan_for(want, poses[0]), poses


def nonfinite_scan():
    """The room case's scan with NaN, +inf and −inf points inside it: (case, rows of the non-finite points)."""
    c = room()
    s = c["scan"][:1500].copy()
    s[7] = (np.nan, 1.0, 2.0)
    s[300] = (np.inf, 0.0, 0.0)
    s[301] = (0.0, -np.inf, 1.0)
    s[1499] = (1.0, 2.0, np.nan)
    c["scan"], c["want"] = s, c["want"][:1500]
    return c, np.array([7, 300, 301, 1499])


FINISH_EPS = 1e-4  # IcpOptions::eps of the finishing scans: the default of 1e-2 ends every one of them after two or three iterations


def finishing_scans():
    """(map, scans, init poses): four room scans; the last starts at the pose that generated it (converged at once), the others
    0.02 m, 0.1 m and 0.4 m off."""
    m = room_map()
    rng = np.random.RandomState(131)
    true = TILT
    scans = [scan_for(_near(rng, m, 1200 + 100 * i, 0.005), true) for i in range(4)]
    inits = np.stack([true] * 4)
    inits[0, 2] += 0.004
    inits[0, :4] /= np.linalg.norm(inits[0, :4])
    inits[0, 4:] += [0.08, -0.07, 0.05]
    inits[1, 4:] += [0.02, -0.01, 0.01]
    inits[2, 4:] += [0.30, -0.25, 0.12]
    return m, scans, inits
