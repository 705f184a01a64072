"""Designed voxels for the NDT voxel records (ndt_voxel_record of csrc/ndt_ingest.hpp, inc_stats_kernel of csrc/ndt_inc.hip), shared by
tests/test_ndt_voxel_ref.py (CPU) and tests/test_gpu_ndt_voxels.py (GPU). Every case is a small cloud whose points all fall in one voxel
of its own; the cases of a target are joined into one shuffled cloud with at least one empty voxel between any two of them, so the
points of a voxel reach the kernel interleaved with everybody else's and in the order the reference (tests/ndt_voxel_ref.py) takes
them. Nothing here calls the library under test or the oracle; everything comes from seeded generators.

family             what it holds
plane ladder       40 points in a tilted box (normal not axis-aligned), half-width 0.14 m in the plane, uniform noise of standard deviation
                   1e-1, 3e-2, 1e-2 … 1e-7 m along the normal, three tilts per rung: lam2/lam0 on both sides of the 1e-3 clamp
line ladder        the same with two small axes, and finer rungs (an eighth of a decade) between 1e-6 and 1e-7 m
clamp edge         lam2/lam0 (lam1 comfortable) or lam1/lam0 (lam2 clamped) within 1e-6 relative of 1e-3, on either side: the points are
                   scaled along one axis until the float32 cloud's own ratio lands there
equal values       cube corners plus centre copies (S proportional to I) and a square prism (two equal, one apart), axis-aligned (dyadic: the equality
                   is exact) and tilted (equal to float32 rounding)
placement          ladder rungs 500 m and 100 000 m out on every axis, in the all-negative octant, and in the double-width cells that touch 0
counts             4 and 5 points (the smallest kept voxels), 1 024 and 4 096 points
coplanar           dyadic coordinates on x + y + 2z = c, 7 … 39 points: lam2 = 0 in exact arithmetic
rank 1             exactly collinear dyadic points; in the min_pts_in_voxel = 1 target two- and three-point voxels
coincident         six copies of one point
incremental only   everything above at voxel size 1 plus one-point voxels, and a second call that returns to voxels of the first (their
                   records are recomputed from that call's points alone, a single point included); the ladders again at voxel size 30
                   (kappa_i up to 3.5e4)

Targets: `main` (direct, min_pts_in_voxel 3), `tiny` (direct, min_pts_in_voxel 1), `inc1` (incremental, voxel size 1, two calls), `inc30`
(incremental, voxel size 30)."""
import functools
from collections import OrderedDict

import numpy as np

import ndt_voxel_ref as ref

N_PTS = 40
EXT = 0.14
HALF_DECADES = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7, 1e-7)
FINE = tuple(1e-6 * 10.0 ** (-k / 8.0) for k in range(1, 8))  # between 1e-6 and 1e-7
TILTS = 3
COPLANAR_N = (7, 8, 9, 11, 13, 16, 19, 23, 27, 31, 35, 39)
BAR_FACTOR = 8.0  # over the oracle's own error, as in the other per-item tests

LONG_N = 1024  # from here on a voxel's sequential sums carry an error that grows with n (up to n·u); every other case has at most 40 points

# The measure is E / (u·kappa), E = max|info - ref| / max|ref|, and the cases fall into groups that are told apart from the 60-digit
# spectrum alone (group_of):
#   direct       at most lam2 clamped (lam1 >= 1e-3 lam0), n <= 40: kappa = kappa_c = lam0 / max(lam2, 1e-3 lam0)
#   direct line  lam1 AND lam2 clamped: kappa = lam0 / lam1. The columns a1, a2 of the one-sided Jacobi carry an absolute error of
#                u·lam0 inside span(v1, v2) against a length of lam1, so U = a/|a| is turned against V inside that plane by about
#                u·lam0/lam1, and V diag(1000/lam0) U^T holds that rotation (an antisymmetric error) instead of the identity. kappa_c
#                = 1000 does not see it: in that measure the oracle's worst is 4.8e7 (E = 5.4e-6, line 1e-07 #2, lam1/lam0 = 4.1e-12).
#                The two measures agree at lam1 = 1e-3 lam0.
#   direct long  n >= 1024: kappa_c; the unit is the sums' own error (about 0.1 n)
#   inc          kappa_i1 = (lam0 + 1e-3)/(lam1 + 1e-3) < 10, n <= 40: kappa = kappa_i = (lam0 + 1e-3)/(lam2 + 1e-3)
#   inc line     kappa_i1 >= 10: kappa_i. The determinant of the cofactor inverse is a sum of terms of size lam0³ that cancels to
#                (lam0 + 1e-3)(lam1 + 1e-3)(lam2 + 1e-3): with two small values the error is u·kappa_i·kappa_i1, beyond kappa_i (voxel
#                size 30: kappa_i1 up to 3e4). A factor below 10 is about the bar's own factor of 8, so the group starts at 10.
#   inc long     n >= 1024: kappa_i
# A unit is the ORACLE's worst figure in its group, over the full-rank cases of `main` and `tiny` (direct) and over every case of
# `inc1` and `inc30` (the incremental record is defined for all of them), never below 1: measured and printed by
# test_ndt_voxel_ref.py::test_units_of_the_oracle, which asserts that the figures here are not below what it measures and within 10 %
# of it (recorded: the measurement rounded up). The GPU's bar is BAR_FACTOR units of the case's group. Every group's unit is at most
# the worst over all groups, so no case is held to less than one bar for everything would hold it to.
UNIT = {"direct": 3.1, "direct line": 1.0, "direct long": 360.0, "inc": 1.71, "inc line": 970.0, "inc long": 53.0}


def group_of(t, c, r):
    """(group, kappa) of a case under target t, or (None, None) where the target's record has no reference (a direct record that is
    not full rank: deficient_verdict)."""
    n = len(c["points"])
    if t["method"] == 2:
        if n == 1:
            return "inc", 1.0
        k1 = float((r["lam"][0] + ref.INC_EPS) / (r["lam"][1] + ref.INC_EPS))
        return ("inc long" if n >= LONG_N else ("inc line" if k1 >= 10.0 else "inc")), float(r["kappa_i"])
    if r["class"] != "full":
        return None, None
    if n >= LONG_N:
        return "direct long", float(r["kappa_c"])
    if r["lam"][1] < ref.CLAMP * r["lam"][0]:
        return "direct line", float(r["lam"][0] / r["lam"][1])
    return "direct", float(r["kappa_c"])


# ---------------------------------------------------------------------------------------------- shapes
def _tilt(rng):
    """A rotation whose third column (the plane's normal) and first column (the line's direction) have no component below 0.2."""
    while True:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        if (np.abs(q[:, 2]) > 0.2).all() and (np.abs(q[:, 0]) > 0.2).all():
            return q


def _box(rng, n, centre, half, R=None):
    """n float32 points: centre + R · (uniform in ±half per axis)."""
    t = rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(half, dtype=np.float64)
    if R is not None:
        t = t @ R.T
    return (np.asarray(centre, dtype=np.float64) + t).astype(np.float32)


SQ3 = np.sqrt(3.0)  # a uniform variable of half-width h has standard deviation h / sqrt(3)


def plane(rng, centre, noise, n=N_PTS, ext=EXT):
    return _box(rng, n, centre, (ext, ext, noise * SQ3), _tilt(rng))


def line(rng, centre, noise, n=N_PTS, ext=EXT):
    return _box(rng, n, centre, (ext, noise * SQ3, noise * SQ3), _tilt(rng))


def _ratios64(p):
    """(lam1/lam0, lam2/lam0) of a float32 cloud in double: for the search of the clamp-edge cases only."""
    d = p.astype(np.float64)
    d = d - d.mean(axis=0)
    w = np.linalg.eigvalsh(d.T @ d)
    return w[1] / w[2], w[0] / w[2]


def clamp_edge(rng, centre, which, delta):
    """40 points whose lam_which/lam0 is 1e-3·(1 + delta) within 2e-7 relative (in double; test_ndt_voxel_ref.py asserts it at 60 digits):
    an axis-aligned box scaled along axis `which`, then tuned by single float32 steps. which = 2: lam1 comfortable; which = 1: lam2 = 1e-5·lam0, clamped."""
    half = (EXT, 0.1, EXT * 0.03) if which == 2 else (EXT, EXT * 0.03, EXT * 0.003)
    t = rng.uniform(-1.0, 1.0, (N_PTS, 3)) * half
    c = np.asarray(centre, dtype=np.float64)
    want = 1e-3 * (1.0 + delta)

    def cloud(s):
        q = t.copy()
        q[:, which] *= s
        return (c + q).astype(np.float32)

    s0 = 1.0
    for _ in range(4):
        s0 *= np.sqrt(want / _ratios64(cloud(s0))[which - 1])
    best = cloud(s0)
    best_err = abs(_ratios64(best)[which - 1] / want - 1.0)
    # float32 rounding makes the ratio a staircase in s with steps far above 1e-6: from the scaled cloud on, single coordinates along
    # that axis move by one float32 step at a time, whichever move brings the ratio nearest
    for _ in range(400):
        if best_err < 2e-7:
            break
        trial, trial_err = None, best_err
        for i in range(N_PTS):
            for to in (-np.inf, np.inf):
                p = best.copy()
                p[i, which] = np.nextafter(p[i, which], np.float32(to))
                err = abs(_ratios64(p)[which - 1] / want - 1.0)
                if err < trial_err:
                    trial, trial_err = p, err
        if trial is None:
            break
        best, best_err = trial, trial_err
    assert best_err < 2e-7, best_err
    return best


def cube(centre, h, copies, R=None):
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) * np.asarray(h, dtype=np.float64)
    if R is not None:
        corners = corners @ R.T
    c = np.asarray(centre, dtype=np.float64)
    return np.vstack([c + corners, np.tile(c, (copies, 1))]).astype(np.float32)


def coplanar(rng, voxel, n):
    """n distinct points of `voxel` (all coordinates >= 1) with dyadic offsets on x + y + 2z = const: exact in float32, lam2 = 0."""
    ij = set()
    while len(ij) < n:
        ij.add((int(rng.randint(10, 55)), int(rng.randint(10, 55))))
    ij = np.array(sorted(ij), dtype=np.float64)[rng.permutation(n)]
    off = np.stack([ij[:, 0] / 64.0, ij[:, 1] / 64.0, (1.75 - (ij[:, 0] + ij[:, 1]) / 64.0) / 2.0], axis=1)
    p = np.asarray(voxel, dtype=np.float64) + off
    assert (p.astype(np.float32).astype(np.float64) == p).all()
    return p.astype(np.float32)


def collinear(rng, voxel, n):
    """n distinct exactly collinear dyadic points of `voxel`: base + t·(2, 1, -1)/128, t integer."""
    t = rng.permutation(np.arange(-20, 21))[:n].astype(np.float64)
    p = np.asarray(voxel, dtype=np.float64) + np.array([0.5, 0.5, 0.5]) + t[:, None] * np.array([2.0, 1.0, -1.0]) / 128.0
    assert (p.astype(np.float32).astype(np.float64) == p).all()
    return p.astype(np.float32)


# ---------------------------------------------------------------------------------------------- where the cases go
@functools.lru_cache(maxsize=None)
def _odd_cells():
    """The voxels with odd coordinates 1 … 15, nearest the origin first: float32 rounding is smallest there, and no two share a face."""
    r = np.arange(1, 16, 2)
    c = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    return c[np.lexsort((c[:, 2], c[:, 1], c[:, 0], c.sum(axis=1), c.max(axis=1)))]


class _Builder:
    def __init__(self, voxel_size=1.0):
        self.vs = float(voxel_size)
        self.cases = OrderedDict()
        self.next_cell = 0

    def cell(self):
        v = _odd_cells()[self.next_cell]
        self.next_cell += 1
        return v

    def centre(self, v):
        return (np.asarray(v, dtype=np.float64) + 0.5) * self.vs

    def add(self, name, family, pts):
        assert name not in self.cases
        self.cases[name] = dict(family=family, points=np.ascontiguousarray(pts, dtype=np.float32))


def _ladders(b, seed, tilts=TILTS, fine=True, ext=EXT, decades=HALF_DECADES):
    rng = np.random.RandomState(seed)
    rungs = [("line", s) for s in FINE] if fine else []
    rungs += [(kind, s) for s in decades for kind in ("line", "plane")]
    rungs.sort(key=lambda r: r[1])  # the finest noise in the cells nearest the origin
    for kind, s in rungs:
        for k in range(tilts):
            gen = plane if kind == "plane" else line
            b.add("%s %.3g #%d" % (kind, s, k), "%s ladder" % kind, gen(rng, b.centre(b.cell()), s, ext=ext))


PLACEMENT_RUNGS = (("plane", 1e-2), ("plane", 1e-3), ("line", 1e-2), ("line", 1e-5))


def _placement(b, seed):
    rng = np.random.RandomState(seed)
    for off in (500, 100000):
        for i, (kind, s) in enumerate(PLACEMENT_RUNGS):
            c = np.array([off + 2 * i + 1, off + 1, off + 1], dtype=np.float64) + 0.5
            b.add("%s %.0e at %d m" % (kind, s, off), "placement", (plane if kind == "plane" else line)(rng, c, s))
    for i, (kind, s) in enumerate(PLACEMENT_RUNGS):  # keys (-1 - 2i, -1, -1): truncation toward zero
        c = -(np.array([2 * i + 1, 1, 1], dtype=np.float64) + 0.5)
        b.add("%s %.0e negative octant" % (kind, s), "placement", (plane if kind == "plane" else line)(rng, c, s))
    zero_cells = ((0, 0, 0), (0, 4, 4), (4, 0, 4), (4, 4, 0))  # a zero component: the cell (-1, 1), the points on both sides of 0
    for (kind, s), v in zip(PLACEMENT_RUNGS, zero_cells):
        c = np.array([0.0 if x == 0 else x + 0.5 for x in v])
        b.add("%s %.0e cell %s" % (kind, s, v), "placement", (plane if kind == "plane" else line)(rng, c, s))


def _main_builder():
    b = _Builder()
    erng = np.random.RandomState(14)  # the cells nearest the origin: the finest float32 steps
    for which in (2, 1):
        for delta in (5e-7, -5e-7):
            for k in range(2):
                b.add("edge lam%d %+.0e #%d" % (which, delta, k), "clamp edge", clamp_edge(erng, b.centre(b.cell()), which, delta))
    _ladders(b, 11)
    rng = np.random.RandomState(12)
    b.add("cube", "equal values", cube(b.centre(b.cell()), 0.25, 2))
    b.add("cube tilted", "equal values", cube(b.centre(b.cell()), 0.25, 2, _tilt(rng)))
    b.add("prism", "equal values", cube(b.centre(b.cell()), (0.125, 0.125, 0.375), 0))
    b.add("prism tilted", "equal values", cube(b.centre(b.cell()), (0.125, 0.125, 0.25), 1, _tilt(rng)))
    for n in (4, 5):
        for k in range(4):
            b.add("n=%d #%d" % (n, k), "counts", _box(rng, n, b.centre(b.cell()), (0.3, 0.3, 0.3)))
    for n in (1024, 4096):
        b.add("n=%d blob" % n, "counts", _box(rng, n, b.centre(b.cell()), (0.4, 0.4, 0.4)))
        b.add("n=%d plane" % n, "counts", plane(rng, b.centre(b.cell()), 1e-2, n=n))
    for n in COPLANAR_N:
        b.add("coplanar n=%d" % n, "coplanar", coplanar(rng, b.cell(), n))
    for n in (4, 7, 12):
        b.add("collinear n=%d" % n, "rank 1", collinear(rng, b.cell(), n))
    v = b.cell()
    b.add("coincident", "coincident", np.tile((v + np.array([0.3, 0.6, 0.7])).astype(np.float32), (6, 1)))
    _placement(b, 13)
    return b


def _tiny_builder():
    b = _Builder()
    rng = np.random.RandomState(21)
    for k in range(4):
        b.add("two points #%d" % k, "rank 1", _box(rng, 2, b.centre(b.cell()), (0.3, 0.3, 0.3)))
    for k in range(3):
        b.add("three points #%d" % k, "rank 1", _box(rng, 3, b.centre(b.cell()), (0.3, 0.3, 0.3)))
    b.add("three collinear points", "rank 1", collinear(rng, b.cell(), 3))
    for k in range(2):
        b.add("n=4 #%d" % k, "counts", _box(rng, 4, b.centre(b.cell()), (0.3, 0.3, 0.3)))
    b.add("plane 1e-2", "plane ladder", plane(rng, b.centre(b.cell()), 1e-2))
    return b


def _join(cases, seed):
    cloud = np.vstack([c["points"] for c in cases.values()])
    return np.ascontiguousarray(cloud[np.random.RandomState(seed).permutation(len(cloud))])


def _finish(name, method, voxel_size, min_pts, calls, families):
    """The target's cases as the kernel sees them: per voxel of the LAST call that touched it, that call's points in that call's order."""
    cases = OrderedDict()
    for ci, (cloud, fam) in enumerate(zip(calls, families)):
        keys = ref.keys_of(cloud, voxel_size)
        for cname, c0 in fam.items():
            pts = c0["points"]
            k = ref.keys_of(pts, voxel_size)
            key = tuple(int(x) for x in k[0])
            mine = (keys == k[0]).all(axis=1)
            for other, c in list(cases.items()):
                if c["key"] == key:  # a later call returns to this voxel: the earlier record is replaced
                    del cases[other]
            cases[cname] = dict(family=c0["family"], key=key, points=np.ascontiguousarray(cloud[mine]), call=ci, design=pts)
    return dict(name=name, method=method, voxel_size=float(voxel_size), min_pts=min_pts, calls=calls, cases=cases)


TARGETS = ("main", "tiny", "inc1", "inc30")


@functools.lru_cache(maxsize=None)
def target(name):
    """dict(name, method 1 direct / 2 incremental, voxel_size, min_pts, calls [float32 clouds], cases: name → dict(family, key,
    points — what the voxel's record is computed from, in order —, call, design — the case as generated))."""
    assert name in TARGETS
    if name == "main":
        b = _main_builder()
        return _finish(name, 1, 1.0, 3, [_join(b.cases, 31)], [b.cases])
    if name == "tiny":
        b = _tiny_builder()
        return _finish(name, 1, 1.0, 1, [_join(b.cases, 32)], [b.cases])
    if name == "inc1":
        first = OrderedDict(_main_builder().cases)
        cell = len(first)
        rng = np.random.RandomState(41)
        cells = _odd_cells()
        # tiny's shapes again, in cells of their own, and one-point voxels
        for cname, c in _tiny_builder().cases.items():
            moved = c["points"].astype(np.float64) - np.trunc(c["points"][0].astype(np.float64)) + cells[cell]
            first["tiny " + cname] = dict(family=c["family"], points=moved.astype(np.float32))
            cell += 1
        for k in range(4):
            first["one point #%d" % k] = dict(family="one point", points=_box(rng, 1, cells[cell] + 0.5, (0.4, 0.4, 0.4)))
            cell += 1
        # the second call returns to eight voxels of the first with other points (one of them with a single point) and adds two
        second = OrderedDict()
        back = ["plane 0.01 #0", "line 1e-06 #1", "edge lam2 +5e-07 #0", "cube", "n=4096 blob", "coplanar n=13", "collinear n=7", "one point #0"]
        for i, cname in enumerate(back):
            v = np.trunc(first[cname]["points"][0].astype(np.float64))
            gen = (lambda c: plane(rng, c, 3e-3, n=12)) if i % 2 == 0 else (lambda c: line(rng, c, 1e-4, n=9))
            second["back to " + cname] = dict(family="second call", points=gen(v + 0.5))
        v = np.trunc(first["plane 0.1 #0"]["points"][0].astype(np.float64))
        second["back to plane 0.1 #0 with one point"] = dict(family="second call", points=_box(rng, 1, v + 0.5, (0.3, 0.3, 0.3)))
        for k in range(2):
            second["new in call 2 #%d" % k] = dict(family="second call", points=plane(rng, cells[cell] + 0.5, 1e-2, n=20))
            cell += 1
        return _finish(name, 2, 1.0, None, [_join(first, 33), _join(second, 34)], [first, second])
    b = _Builder(30.0)
    _ladders(b, 51, tilts=1, fine=False, ext=8.5, decades=(3.0, 1.0, 0.3) + HALF_DECADES[:9])  # below 1e-5 m float32 rounding 300 m out takes over
    return _finish(name, 2, 30.0, None, [_join(b.cases, 35)], [b.cases])


@functools.lru_cache(maxsize=None)
def reference(name):
    """name of every case of the target → ref.record of its points (dict; adds 'class')."""
    out = OrderedDict()
    for cname, c in target(name)["cases"].items():
        r = ref.record(c["points"])
        r["class"] = ref.rank_class(r)
        out[cname] = r
    return out


def by_key(t, keys):
    """Row of every case of the target in a dump's key array [n, 3] → dict case name → row; asserts the dump holds exactly the cases'
    voxels."""
    at = {tuple(int(x) for x in k): i for i, k in enumerate(np.asarray(keys))}
    assert len(at) == len(keys) == len(t["cases"]), (len(at), len(keys), len(t["cases"]))
    return {cname: at[c["key"]] for cname, c in t["cases"].items()}


def record_figures(t, refs, rows, mu, info):
    """Per case of a dump (mu [n, 3], info [n, 3, 3], rows from by_key): dict case name → dict(cls, family, group, kappa, fig —
    E/(u kappa) of the target's own record, None where the reference has none —, E, asym, mu_err, mu_bound)."""
    out = OrderedDict()
    for cname, c in t["cases"].items():
        r, i = refs[cname], rows[cname]
        group, kappa = group_of(t, c, r)
        finite = bool(np.isfinite(info[i]).all())
        E = fig = None
        if group is not None:
            E = ref.rel_err(info[i], r["inc"] if t["method"] == 2 else r["direct"]) if finite else np.inf
            fig = E / (ref.U * kappa)
        out[cname] = dict(cls=r["class"], family=c["family"], group=group, kappa=kappa, fig=fig, E=E, asym=ref.asymmetry(info[i]) if finite else np.inf,
                          mu_err=ref.mu_err(mu[i], r), mu_bound=ref.mu_bound(c["points"]))
    return out


def worst_by(figs, by="family", what="fig"):
    """family (or group) → (worst value, the case that set it) over the cases that have a figure."""
    out = OrderedDict()
    for cname, f in figs.items():
        if f[what] is None:
            continue
        if f[by] not in out or f[what] > out[f[by]][0]:
            out[f[by]] = (f[what], cname)
    return out


def coplanar_sign(info, r):
    """An exactly coplanar voxel's record against its two candidates → (sign +1 / -1 of the nearer one, its E/(u·1000), the other's)."""
    plus, minus = ref.candidates(r)
    fp, fm = ref.figure(info, plus, 1000.0), ref.figure(info, minus, 1000.0)
    return (1, fp, fm) if fp <= fm else (-1, fm, fp)


def deficient_verdict(c, r, info, bar):
    """A direct record of a case that is not full rank against the rules of its family → dict(kind, ok, sign, text). `bar` is in the
    measure's units, E / (u·1000): kappa_c is 1000 wherever a value is clamped.
      coplanar    within the bar of T0 + T1 + T2 or of T0 + T1 - T2 (sign: which);
      rank 1      info·v0 and v0^T·info equal v0/lam0 within the bar, every singular value <= 1000/lam0·(1 + bar·u·1000), all entries finite;
      coincident  not finite."""
    info = np.asarray(info, dtype=np.float64)
    if r["class"] == "coincident":
        bad = int((~np.isfinite(info)).sum())
        return dict(kind="coincident", ok=bad > 0, sign=0, text="%d of 9 entries not finite" % bad)
    assert r["class"] == "deficient"
    if c["family"] == "coplanar":
        if not np.isfinite(info).all():
            return dict(kind="coplanar", ok=False, sign=0, text="not finite")
        sign, near, far = coplanar_sign(info, r)
        return dict(kind="coplanar", ok=near <= bar, sign=sign, text="%s v2 v2^T/(1e-3 lam0): %.2f (the other candidate: %.3g; bar %.1f)" % ("+" if sign > 0 else "-", near, far, bar))
    e_r, e_l, s, finite = ref.null_space_checks(info, r)
    tol = bar * ref.U * 1000.0
    return dict(kind="rank 1", ok=bool(finite and e_r <= tol and e_l <= tol and s <= 1.0 + tol), sign=0,
                text="|info v0 - v0/lam0| lam0 = %.2e, |v0^T info - v0^T/lam0| lam0 = %.2e (bar %.2e); largest singular value · lam0/1000 = 1 %+.2e" % (e_r, e_l, tol, s - 1.0))


# ---------------------------------------------------------------------------------------------- the oracle's side (handed in by the tests)
def oracle_target(locref, t, calls=None):
    if t["method"] == 1:
        ndt = locref.Ndt(method=1, voxel_size=t["voxel_size"], min_pts_in_voxel=t["min_pts"])
    else:
        ndt = locref.Ndt(method=2, voxel_size=t["voxel_size"], capacity=100000)
    for c in t["calls"][:calls]:
        ndt.set_target(c)
    return ndt
