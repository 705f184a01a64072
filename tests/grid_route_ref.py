"""Helper of tests/test_grid_route_ref.py, tests/test_gpu_grid_lists.py and test_device_grid_invariants: a plain numpy restatement of
how the exact grid search (csrc/grid_build.hip, csrc/grid_kernels.hip) routes a query — which queries the tile kernel can answer
from its staged 8×8×8-cell block, after which ring, and which it must hand to the tree.

float32 wherever the kernels use float32: the library is built with -ffp-contract=off, so `(v - o) * inv`, floorf and the face
expressions of settle_top round here as they do there. Nothing in this file computes a neighbour LIST: the lists are compared with
the oracle's k-NN; this file only says which path a query takes, so that a test can show its input reaches the path it names.

    grid_dump(api, ctx)     the grid the library built for the current target (locgpu_debug_grid_dump)
    ladder(points)          the grid the build WOULD choose for these (distinct) points — CPU tests of inputs only
    route(grid, q, K)       per query one of CLASSES
"""
import ctypes

import numpy as np

TILE = 4            # kGridTile
STAGE_RING = 2      # kStageRing
STAGE_CAP = 1024    # kStageCap
RANGE_Q = 256       # kRangeQ (and the bin kernels' block size)
TARGET_OCC = 4.0    # grid_build.hip: leaves per occupied cell the ladder stops at

CLASSES = ("outside", "no_tile", "no_fit", "ring1", "ring2", "open", "tie")
TO_TREE_FOR_SURE = ("outside", "no_tile", "no_fit")  # integer decisions on the dumped grid: exact

_F = np.float32
TILE_REC = np.dtype([("pt_start", "<u4"), ("tile_lin", "<u4"), ("cstart", "<u2", (66,))])


def _finish(grid):
    """leaf_cell, tile_lin of a grid given origin, inv_cell, dims, tdims and the leaves."""
    xyz = grid["pts"][:, :3]
    dims = grid["dims"]
    c = np.floor((xyz - grid["origin"]) * grid["inv_cell"]).astype(np.int64)
    c = np.minimum(np.maximum(c, 0), dims - 1)  # cell_key_kernel clamps
    t = c // TILE
    td = grid["tdims"]
    grid["leaf_cell"] = c
    grid["leaf_tile"] = (t[:, 2] * td[1] + t[:, 1]) * td[0] + t[:, 0]
    grid["tile_lin"] = np.unique(grid["leaf_tile"])
    return grid


def grid_dump(api, ctx):
    """The exact-search grid of ctx's current target, built on first use: dict of n (leaves), dims, tdims, n_occ (occupied cells),
    n_tocc (occupied tiles), cap (hash capacity), origin, cell, inv_cell, slack, pts [n, 4] float32 (x, y, z, bits(leaf slot)) in
    (tile, cell) order, tiles (the raw 140-byte records) and hash [cap, 2]; plus leaf_cell / leaf_tile / tile_lin for route()."""
    L = api.lib()
    L.locgpu_debug_grid_dump.restype = ctypes.c_size_t
    L.locgpu_debug_grid_dump.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_void_p, ctypes.c_size_t]
    info = np.zeros(9, np.int64)
    prm = np.zeros(6, np.float32)
    n = L.locgpu_debug_grid_dump(ctx._h, info.ctypes.data, prm.ctypes.data, None, 0, None, 0, None, 0)
    assert n > 0, "no grid (no target, or the build refused it)"
    n_tocc, cap = int(info[4]), int(info[5])
    gp = np.zeros((n, 4), np.float32)
    rec = np.zeros(n_tocc, dtype=TILE_REC)
    assert rec.dtype.itemsize == 140
    hsh = np.zeros((cap, 2), np.uint32)
    L.locgpu_debug_grid_dump(ctx._h, info.ctypes.data, prm.ctypes.data, gp.ctypes.data, gp.size, rec.ctypes.data, rec.nbytes, hsh.ctypes.data, hsh.size)
    return _finish(dict(n=int(n), dims=info[:3].copy(), n_occ=int(info[3]), n_tocc=n_tocc, cap=cap, tdims=info[6:9].copy(), origin=prm[:3].copy(),
                        cell=_F(prm[3]), inv_cell=_F(prm[4]), slack=_F(prm[5]), pts=gp, tiles=rec, hash=hsh))


def ladder(points):
    """The grid grid_build_device chooses for `points` (taken as the tree's leaves: distinct, finite float32 rows): the edge climbs
    from ext / 8192 by factors of 1.3 and stops at the first one with ≥ TARGET_OCC leaves per occupied cell."""
    xyz = np.unique(np.ascontiguousarray(np.asarray(points, dtype=np.float32)[:, :3]), axis=0)
    n = len(xyz)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    ext = max(float(np.max(hi.astype(np.float64) - lo.astype(np.float64))), 1e-3)
    cell = ext
    c = ext / 8192.0
    while c < ext:
        inv = _F(1.0 / c)
        k = np.maximum((xyz - lo) * inv, _F(0)).astype(np.int64)  # probe_key_kernel: truncation of the float32 product
        occ = len(np.unique((k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]))
        cell = c
        if n / occ >= TARGET_OCC:
            break
        c *= 1.3
    cellf = _F(cell)
    inv = _F(1.0) / cellf
    dims = np.floor((hi - lo) * inv).astype(np.int64) + 1
    tdims = (dims + TILE - 1) // TILE
    max_abs = _F(0)
    for a in range(3):
        max_abs = max(max_abs, max(abs(lo[a]), abs(lo[a] + _F(dims[a]) * cellf)))
    slack = _F(1e-3) * cellf + _F(16.0) * _F(1.2e-7) * _F(max_abs)
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = xyz
    g = _finish(dict(n=n, dims=dims, tdims=tdims, origin=lo.copy(), cell=cellf, inv_cell=inv, slack=_F(slack), pts=pts))
    g["n_tocc"] = len(g["tile_lin"])
    g["n_occ"] = len(np.unique(g["leaf_tile"] * 64 + ((g["leaf_cell"][:, 2] % 4) * 4 + g["leaf_cell"][:, 1] % 4) * 4 + g["leaf_cell"][:, 0] % 4))
    return g


def query_cells(grid, queries):
    """(inside [n] bool, cell [n, 3] int64 — valid where inside, tile key [n] int64 — tile_lin, or -1 outside): grid_bin_count_kernel's
    cell_coord and range test. A coordinate whose float32 cell number is out of range — ±inf and 1e17 included — is outside."""
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32)[:, :3])
    dims, td = grid["dims"], grid["tdims"]
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((q - grid["origin"]) * grid["inv_cell"])
        inside = np.all((f >= 0) & (f < dims.astype(np.float32)), axis=1) & ~np.isnan(q).any(axis=1)
    c = np.where(inside[:, None], f, 0).astype(np.int64)
    t = c // TILE
    lin = np.where(inside, (t[:, 2] * td[1] + t[:, 1]) * td[0] + t[:, 0], -1)
    return inside, c, lin


def block_leaves(grid, lin):
    """Indices (into grid['pts']) of the leaves tile `lin`'s staged block holds: its 4×4×4 cells and two rings of cells around them."""
    td = grid["tdims"]
    t = np.array([lin % td[0], (lin // td[0]) % td[1], lin // (td[0] * td[1])], dtype=np.int64)
    lc = grid["leaf_cell"]
    return np.nonzero(np.all((lc >= TILE * t - STAGE_RING) & (lc <= TILE * t + TILE - 1 + STAGE_RING), axis=1))[0]


def _settle(grid, q, c, full, top, R):
    """settle_top after ring R: 0 = final, 1 = more rings needed, 2 = every leaf examined and fewer than K exist."""
    o, cell, slack, dims = grid["origin"], grid["cell"], grid["slack"], grid["dims"]
    m = len(q)
    dmin = np.full(m, np.inf, np.float32)
    open_face = np.zeros(m, bool)
    for a in range(3):
        is_open = c[:, a] - R > 0
        v = q[:, a] - (o[a] + (c[:, a] - R).astype(np.float32) * cell)
        dmin = np.where(is_open, np.fmin(dmin, v), dmin)
        open_face |= is_open
        is_open = c[:, a] + R < dims[a] - 1
        v = (o[a] + (c[:, a] + R + 1).astype(np.float32) * cell) - q[:, a]
        dmin = np.where(is_open, np.fmin(dmin, v), dmin)
        open_face |= is_open
    with np.errstate(invalid="ignore"):
        safe = dmin - slack
        settled = full & (safe > 0) & (top <= safe * safe)
    assert safe.dtype == np.float32
    return np.where(open_face, np.where(settled, 0, 1), np.where(full, 0, 2))


def _smallest(d2, mask, K):
    """The K + 1 smallest of every row of d2 where mask, ascending, +inf where a row has fewer."""
    x = np.where(mask, d2, np.float32(np.inf))
    if x.shape[1] < K + 1:
        x = np.concatenate([x, np.full((x.shape[0], K + 1 - x.shape[1]), np.inf, np.float32)], axis=1)
    return np.sort(x, axis=1)[:, :K + 1]


def route(grid, queries, K, detail=False):
    """Per query (float32 coordinates in the map frame, as the kernels see them) one of CLASSES, as an array of str.

    outside, no_tile and no_fit are integer decisions and exact; ring1, ring2 and open follow settle_top in float32. `tie` is a lower
    bound on the kernel's flag: the kernel also flags a candidate that equals the K-th distance at the moment it is offered, whatever
    becomes of that distance later. detail=True returns (classes, may_tie): may_tie marks the ring1 / ring2 queries among whose
    examined candidates two float32 distances are equal — every flag TopK raises needs such a pair, so the queries the stage hands
    to the tree number at least outside + no_tile + no_fit + open + tie and at most that plus may_tie (walked_bounds)."""
    q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32)[:, :3])
    inside, c, lin = query_cells(grid, q)
    out = np.full(len(q), "outside", dtype="<U8")
    may_tie = np.zeros(len(q), bool)
    has = inside & np.isin(lin, grid["tile_lin"])
    out[inside & ~has] = "no_tile"
    xyz = grid["pts"][:, :3]
    inf = np.float32(np.inf)
    for t in np.unique(lin[has]):
        sel = np.nonzero(has & (lin == t))[0]
        blk = block_leaves(grid, int(t))
        if len(blk) > STAGE_CAP:
            out[sel] = "no_fit"
            continue
        qs, cs = q[sel], c[sel]
        d = qs[:, None, :] - xyz[blk][None, :, :]
        d2 = d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])  # Eigen squaredNorm order
        assert d2.dtype == np.float32
        cheb = np.abs(grid["leaf_cell"][blk][None, :, :] - cs[:, None, :]).max(axis=2)
        s1 = _smallest(d2, cheb <= 1, K)
        o1 = _settle(grid, qs, cs, s1[:, K - 1] < inf, s1[:, K - 1], 1)
        s2 = _smallest(d2, cheb <= 2, K)
        o2 = _settle(grid, qs, cs, s2[:, K - 1] < inf, s2[:, K - 1], 2)
        more = o1 == 1
        s = np.where(more[:, None], s2, s1)
        outcome = np.where(more, o2, o1)
        tie = (s[:, K - 1] == s[:, K]) & (s[:, K - 1] < inf)
        for j in range(K - 1):
            tie |= (s[:, j] == s[:, j + 1]) & (s[:, j] < inf)
        out[sel] = np.where(outcome != 0, "open", np.where(tie, "tie", np.where(more, "ring2", "ring1")))
        seen = np.sort(np.where(cheb <= np.where(more, 2, 1)[:, None], d2, inf), axis=1)
        may_tie[sel] = np.any((seen[:, 1:] == seen[:, :-1]) & (seen[:, 1:] < inf), axis=1) & (outcome == 0) & ~tie
    return (out, may_tie) if detail else out


def walked_bounds(classes, may_tie):
    """(least, most) queries the grid stage hands to the tree."""
    least = int(sum(np.sum(classes == k) for k in TO_TREE_FOR_SURE + ("open", "tie")))
    return least, least + int(np.sum(may_tie))


def shares(classes):
    """{class: count} over CLASSES."""
    return {k: int(np.sum(classes == k)) for k in CLASSES}


def to_tree_for_sure(classes):
    return int(sum(np.sum(classes == k) for k in TO_TREE_FOR_SURE))


def fmt(classes):
    n = max(len(classes), 1)
    return " ".join("%s %d (%.1f%%)" % (k, v, 100.0 * v / n) for k, v in shares(classes).items() if v)
