"""Designed inputs for the NDT voxel hash tables and their CPU-side facts, shared by tests/test_ndt_table_cases_ref.py (CPU) and
tests/test_gpu_ndt_tables.py (GPU). The small world runs the tables at load 0.03, where a collision walk is rare and short; here the
collisions are chosen: the key rules of csrc/ndt_key.hpp and csrc/ndt_set_key.hpp are restated in numpy, the voxels 1 … 160 per axis are
searched for keys whose first slot falls in the last few slots of the table, and dozens of them make one chain that runs through the
end of the table. Nothing here calls the library under test, and the oracle only where a test hands it in; everything comes from seeded
generators; voxel size 1.0.

What is restated here and must follow the code: ndt_pack, ndt_hash, ndt_hash32 (csrc/ndt_key.hpp), ndt_set_pack (csrc/ndt_set_key.hpp),
the sizing of ndt_table_alloc (csrc/ndt_kernels.hip: direct table and voxel set) and of rebuild_table_and_stats (csrc/ndt_inc.hip).
tests/test_ndt_table_cases_ref.py compares the packs and hashes with the host harness tests/cpp/ndt_key_check.cpp, and the table tests
compare the slot counts and every key's probe path with the device's."""
import functools
from collections import OrderedDict

import numpy as np

U64 = np.uint64
EMPTY = U64(0xFFFFFFFFFFFFFFFF)  # kNdtEmpty
BIAS = 1 << 20                   # kNdtBias
SET_BIAS = 1 << 15               # kNdtSetBias
LATTICE = 160                    # the voxels 1 … 160 per axis are searched
MIN_PTS = 3                      # NdtOptions::min_pts_in_voxel_: a direct voxel is kept with MORE points than this
# Every residual that is found is accepted under this gate, so the number of accepted (point, voxel) pairs of a point is the number of
# its probes that HIT: a look-up that misses a chained voxel changes an exact count. (The gate itself is tested in test_gpu_ndt_hb.py.)
RES_TH = 1.0e6
NEARBY = np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1)], dtype=np.int64)  # nearby_grids_ order

# The per-point unit on the designed queries: the ORACLE's worst per-point H and B error against ndt_hb_ref.per_point, measured and
# printed by test_ndt_table_cases_ref.py::test_per_point_unit_of_the_oracle_on_the_designed_queries, which also asserts that these
# figures are not below what it measures (recorded: the measurement rounded up to two digits). method → (H, B); the GPU's bar is
# ndt_hb_cases.BAR_FACTOR (8) units.
UNIT = {1: (4.4e-16, 3.7e-14), 2: (7.6e-16, 1.13e-12)}


# ---------------------------------------------------------------------------------------------- the key rules
def ndt_pack(k):
    """ndt_pack: 21 bits per axis, biased by 2^20. k [..., 3] int → uint64."""
    k = np.asarray(k, dtype=np.int64)
    assert (np.abs(k) < BIAS).all()
    b = (k + BIAS).astype(U64)
    return (b[..., 0] << U64(42)) | (b[..., 1] << U64(21)) | b[..., 2]


def ndt_set_pack(target, k):
    """ndt_set_pack under ndt_set_target_bits(target): target:16 | x:16 | y:16 | z:16, biased by 2^15."""
    k = np.asarray(k, dtype=np.int64)
    assert (np.abs(k) < SET_BIAS).all() and 0 <= int(target) < 65535
    b = (k + SET_BIAS).astype(U64)
    return (U64(int(target)) << U64(48)) + (b[..., 0] << U64(32)) + (b[..., 1] << U64(16)) + b[..., 2]


def ndt_hash(key, cap):
    """ndt_hash (the incremental table): the 64-bit murmur finaliser, low bits."""
    k = np.array(key, dtype=U64, copy=True, ndmin=1)
    k ^= k >> U64(33)
    k *= U64(0xff51afd7ed558ccd)
    k ^= k >> U64(33)
    k *= U64(0xc4ceb9fe1a85ec53)
    k ^= k >> U64(33)
    return (k & U64(cap - 1)).astype(np.int64)


def ndt_hash32(key, cap):
    """ndt_hash32 (direct table and voxel set): the halves of the key folded with one multiply, then the 32-bit murmur finaliser."""
    key = np.atleast_1d(np.asarray(key, dtype=U64))
    lo = (key & U64(0xFFFFFFFF)).astype(np.uint32)
    hi = (key >> U64(32)).astype(np.uint32)
    h = lo + hi * np.uint32(0x9E3779B1)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85ebca6b)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xc2b2ae35)
    h ^= h >> np.uint32(16)
    return (h.astype(np.int64)) & (cap - 1)


def unpack(key):
    """The voxel of an ndt_pack key (ndt_dump_kernel's rule) → [..., 3] int64."""
    key = np.asarray(key, dtype=U64)
    m = U64(0x1FFFFF)
    return np.stack([(key >> U64(42)) & m, (key >> U64(21)) & m, key & m], axis=-1).astype(np.int64) - BIAS


# ---------------------------------------------------------------------------------------------- the capacity rules
def direct_capacity(runs):
    """ndt_table_alloc: the smallest power of two >= max(1024, 32 x runs) (at most 2^26 by that rule) and never below 2 x runs; `runs`
    counts every voxel run of the cloud — for a set of all targets together — the dropped ones included."""
    cap = 1024
    while cap < 32 * runs and cap < (1 << 26):
        cap <<= 1
    while cap < 2 * runs:
        cap <<= 1
    return cap


def inc_capacity(live, have=0):
    """rebuild_table_and_stats: the smallest power of two >= max(1024, 2 x live); the table only grows (`have`: its size before)."""
    cap = 1024
    while cap < 2 * max(live, 1):
        cap <<= 1
    return max(cap, have)


# ---------------------------------------------------------------------------------------------- linear probing
def probe_sim(homes, cap):
    """Linear probing of keys with first slots `homes` into `cap` slots. Returns (occupied [cap] bool — it does not depend on the order
    of insertion — and per key its worst-case displacement: where it lands when every other key went in before it)."""
    homes = np.asarray(homes, dtype=np.int64)
    assert len(homes) < cap

    def fill(hs):
        occ = np.zeros(cap, bool)
        for h in hs:
            while occ[h]:
                h = (h + 1) & (cap - 1)
            occ[h] = True
        return occ

    occ = fill(homes)
    disp = np.zeros(len(homes), dtype=np.int64)
    for i, h in enumerate(homes):
        if not occ[(h + 1) & (cap - 1)] and (homes == h).sum() == 1 and not occ[(h - 1) & (cap - 1)]:
            continue  # alone in its cluster: displacement 0 whatever the order
        others = fill(np.delete(homes, i))
        d = 0
        while others[(h + d) & (cap - 1)]:
            d += 1
        disp[i] = d
    return occ, disp


def wrap_run(occ):
    """The slots of the maximal run of occupied slots that crosses cap − 1 → 0, in walk order; empty when there is none."""
    cap = len(occ)
    if not (occ[cap - 1] and occ[0]) or occ.all():
        return np.zeros(0, np.int64)
    a = cap - 1
    while occ[a - 1]:
        a -= 1
    b = 0
    while occ[b + 1]:
        b += 1
    return np.concatenate([np.arange(a, cap), np.arange(0, b + 1)])


# ---------------------------------------------------------------------------------------------- points
def points_in_voxel(rng, voxel, m, lo=0.1, hi=0.9):
    """m float32 points strictly inside `voxel` (positive coordinates only: voxel 0 is double width under truncation)."""
    v = np.asarray(voxel, dtype=np.float64)
    assert (v >= 1).all()
    p = (v + rng.uniform(lo, hi, (m, 3))).astype(np.float32)
    assert (np.trunc(p.astype(np.float64)) == v).all()
    return p


def voxels_of(points):
    return np.trunc(np.asarray(points, dtype=np.float32).astype(np.float64)[:, :3]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def lattice():
    r = np.arange(1, LATTICE + 1, dtype=np.int64)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)


def _tuples(v):
    return {tuple(int(c) for c in r) for r in np.asarray(v).reshape(-1, 3)}


def face_adjacent_pairs(vox):
    """Index pairs (i, j), i < j, of voxels [n, 3] that share a face."""
    at = {tuple(v): i for i, v in enumerate(np.asarray(vox).tolist())}
    out = []
    for v, i in at.items():
        for ax in range(3):
            w = list(v)
            w[ax] += 1
            j = at.get(tuple(w))
            if j is not None:
                out.append((min(i, j), max(i, j)))
    return out


def build_queries(rng, present, slots_of, cap, per_voxel, skip=(), n_front=12, n_behind=24, n_neigh=20, dropped=()):
    """Queries against a table that holds the voxels `present` [n, 3] (slots_of: voxels → first slots in `cap` slots):
    per_voxel(v) → points in the present voxel v; then points in ABSENT voxels whose first slot lies inside the occupied run that
    crosses the end of the table — n_front of them in front of the wrap, so that the miss is found only at the chain's end, n_behind
    behind it; points in the `dropped` voxels; and n_neigh points whose centre voxel is absent but whose face neighbour is a present voxel
    of the chain. `skip`: voxels that may not serve as absent ones. Returns dict(points float32 [n, 3], kind name → row indices,
    absent [a, 3] the absent voxels used)."""
    present = np.asarray(present, dtype=np.int64)
    homes = slots_of(present)
    occ, _ = probe_sim(homes, cap)
    run = wrap_run(occ)
    assert len(run) >= 2
    inside = np.zeros(cap, bool)
    inside[run] = True
    taken = _tuples(present) | _tuples(skip) | _tuples(dropped)
    lat = lattice()
    lh = slots_of(lat)
    pool = [i for i in np.flatnonzero(inside[lh]) if tuple(lat[i].tolist()) not in taken]
    pool = np.array(pool, dtype=np.int64)[rng.permutation(len(pool))]
    front = [i for i in pool if lh[i] >= cap // 2][:n_front]
    behind = [i for i in pool if lh[i] < cap // 2][:n_behind]
    assert len(front) == n_front and len(behind) == n_behind
    rows, kind = [], {}

    def add(name, pts):
        at = sum(len(r) for r in rows)
        rows.append(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
        kind[name] = np.concatenate([kind.get(name, np.zeros(0, np.int64)), np.arange(at, at + len(rows[-1]))])

    for v in present:
        add("present", per_voxel(v))
    for i in front:
        add("absent_front", points_in_voxel(rng, lat[i], 1))
    for i in behind:
        add("absent_behind", points_in_voxel(rng, lat[i], 1))
    for v in np.asarray(dropped, dtype=np.int64).reshape(-1, 3):
        add("dropped", points_in_voxel(rng, v, 2))
    absent = [lat[i] for i in front + behind]
    # a present voxel of the chain, seen from the absent voxel across one of its faces: the point sits 0.05 … 0.15 from that face
    chain = [v for v, h in zip(present, homes) if inside[h]]
    faces = [(v, ax, d) for v in chain for ax in range(3) for d in (-1, 1)]
    faces = [faces[i] for i in rng.permutation(len(faces))]
    faces = [(v, ax, d) for v, ax, d in faces if v[ax] + d >= 1 and tuple((v + d * np.eye(3, dtype=np.int64)[ax]).tolist()) not in taken]
    assert faces
    used = 0
    while used < n_neigh:  # every face once before any face twice
        v, ax, d = faces[used % len(faces)]
        n = v.copy()
        n[ax] += d
        off = rng.uniform(0.2, 0.8, 3)
        off[ax] = rng.uniform(0.05, 0.15) if d == 1 else rng.uniform(0.85, 0.95)
        p = (n + off).astype(np.float32)
        assert (np.trunc(p.astype(np.float64)) == n).all()
        add("neighbour", p)
        absent.append(n)
        used += 1
    assert used == n_neigh
    return dict(points=np.ascontiguousarray(np.vstack(rows)), kind=kind, absent=np.array(absent, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- direct cases
DIRECT_CAP = 2048
DIRECT_TAIL = 8  # first slots in the last 8 slots
DIRECT_CASES = ("end_chain", "same_slot", "dropped_in_chain")


def _direct_slots(v):
    return ndt_hash32(ndt_pack(v), DIRECT_CAP)


@functools.lru_cache(maxsize=None)
def direct_case(name):
    """dict(cloud float32 [n, 3], kept [48, 3], dropped [d, 3], runs, cap, queries (build_queries), poses)."""
    assert name in DIRECT_CASES
    rng = np.random.RandomState({"end_chain": 101, "same_slot": 102, "dropped_in_chain": 101}[name])
    lat = lattice()
    home = _direct_slots(lat)
    if name == "same_slot":
        last = np.flatnonzero(home == DIRECT_CAP - 1)
        kept = np.concatenate([lat[last[rng.permutation(len(last))[:3]]], lat[rng.permutation(len(lat))[:45]]])
    else:
        tail = lat[home >= DIRECT_CAP - DIRECT_TAIL]
        pairs = face_adjacent_pairs(tail)
        chosen, members = [], set()
        for i, j in (pairs[k] for k in rng.permutation(len(pairs))):
            if i not in members and j not in members and len(chosen) < 6:
                chosen.append((i, j))
                members.update((i, j))
        rest = [i for i in rng.permutation(len(tail)) if i not in members][:48 - len(members)]
        kept = tail[sorted(members) + rest]
    assert len(_tuples(kept)) == 48
    dropped = np.zeros((0, 3), np.int64)
    if name == "dropped_in_chain":
        occ, _ = probe_sim(_direct_slots(kept), DIRECT_CAP)
        inside = np.zeros(DIRECT_CAP, bool)
        inside[wrap_run(occ)] = True
        cand = [i for i in np.flatnonzero(inside[home]) if tuple(lat[i].tolist()) not in _tuples(kept)]
        cand = [cand[i] for i in np.random.RandomState(103).permutation(len(cand))]
        dropped = np.array([lat[next(i for i in cand if home[i] >= DIRECT_CAP // 2)], lat[next(i for i in cand if home[i] < DIRECT_CAP // 2)]])
    cloud = np.vstack([points_in_voxel(rng, v, 8) for v in kept] + [points_in_voxel(rng, v, MIN_PTS) for v in dropped])
    cloud = np.ascontiguousarray(cloud[rng.permutation(len(cloud))])
    runs = len(kept) + len(dropped)
    qrng = np.random.RandomState(7)
    if name == "dropped_in_chain":
        q = build_queries(qrng, kept, _direct_slots, DIRECT_CAP, lambda v: points_in_voxel(qrng, v, 4), dropped=dropped)
    else:  # the voxels dropped_in_chain drops are plain absent voxels here, and queried all the same
        q = build_queries(qrng, kept, _direct_slots, DIRECT_CAP, lambda v: points_in_voxel(qrng, v, 4), dropped=direct_case("dropped_in_chain")["dropped"]
                          if name == "end_chain" else ())
    return dict(cloud=cloud, kept=kept, dropped=dropped, runs=runs, cap=direct_capacity(runs), queries=q)


SMALL_POSE = np.array([1.5e-5, -1.0e-5, 2.0e-5, 0.0, 0.004, -0.003, 0.002])  # tens of microradians (160 m out: millimetres) and millimetres: nearly every query stays in its voxel
SMALL_POSE[3] = np.sqrt(1.0 - (SMALL_POSE[:3] ** 2).sum())
IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])


# ---------------------------------------------------------------------------------------------- the set case
SET_CAP = 4096
SET_TAIL = 64
SET_TARGETS = 3


@functools.lru_cache(maxsize=None)
def set_case():
    """Three targets in one table of 4 096 slots. Targets 0 and 2 hold the same 24 coordinate triples (different points) — triples
    whose key lands in the last 64 slots under BOTH targets — and 16 voxels of their own there; target 1 holds none of the shared
    triples but 40 other voxels of the same region. dict(clouds [3], voxels [3] of [40, 3], shared [24, 3], runs, cap, keys [3] uint64,
    scans [3] float32: two points in every coordinate triple any target holds)."""
    rng = np.random.RandomState(201)
    lat = lattice()
    tail = [ndt_hash32(ndt_set_pack(t, lat), SET_CAP) >= SET_CAP - SET_TAIL for t in range(SET_TARGETS)]
    both = np.flatnonzero(tail[0] & tail[2])
    shared = lat[both[rng.permutation(len(both))[:24]]]
    taken = _tuples(shared)
    voxels = []
    for t in range(SET_TARGETS):
        own = [i for i in np.flatnonzero(tail[t])[rng.permutation(int(tail[t].sum()))] if tuple(lat[i].tolist()) not in taken][:40 if t == 1 else 16]
        voxels.append(np.concatenate([shared, lat[own]]) if t != 1 else lat[own])
        taken |= _tuples(lat[own])
    clouds = []
    for t in range(SET_TARGETS):
        c = np.vstack([points_in_voxel(rng, v, 8) for v in voxels[t]])
        clouds.append(np.ascontiguousarray(c[rng.permutation(len(c))]))
    everything = np.array(sorted(_tuples(np.vstack(voxels))), dtype=np.int64)
    scans = [np.ascontiguousarray(np.vstack([points_in_voxel(rng, v, 2) for v in everything])) for _ in range(SET_TARGETS)]
    runs = sum(len(v) for v in voxels)
    return dict(clouds=clouds, voxels=voxels, shared=shared, runs=runs, cap=direct_capacity(runs), keys=[ndt_set_pack(t, voxels[t]) for t in range(SET_TARGETS)],
                everything=everything, scans=scans)


# ---------------------------------------------------------------------------------------------- incremental cases
INC_TAIL = 8
INC_CASES = ("lookup_chain", "evict_from_chain", "growth")


def _inc_slots(cap):
    return lambda v: ndt_hash(ndt_pack(v), cap)


def lru_replay(live, cloud, capacity):
    """SetIncNdtTargetCloud's voxel set (ndt_registration.cpp:150-183) point by point: an LRU cache of capacity − 1 voxels. `live`:
    OrderedDict voxel → None, oldest first; changed in place."""
    for v in map(tuple, voxels_of(cloud).tolist()):
        if v in live:
            live.move_to_end(v)
        else:
            live[v] = None
            if len(live) > capacity - 1:
                live.popitem(last=False)
    return live


@functools.lru_cache(maxsize=None)
def inc_case(name):
    """dict(capacity, calls [clouds], live [after each call: sorted [n, 3]], caps [the table's slots after each call], points [after
    each call: voxel tuple → the points its statistics come from], queries (against the last state), chain_tail (cap whose last 8 slots
    the design aims at))."""
    assert name in INC_CASES
    lat = lattice()
    if name == "growth":
        rng = np.random.RandomState(303)
        tail = lat[_inc_slots(2048)(lat) >= 2048 - INC_TAIL]
        tail = tail[rng.permutation(len(tail))[:24]]
        rest = [v for v in lat[rng.permutation(len(lat))[:700]].tolist() if tuple(v) not in _tuples(tail)][:576]
        first = np.concatenate([tail[:16], np.array(rest[:484])])
        second = np.concatenate([tail[16:], np.array(rest[484:])])
        assert len(first) == 500 and len(second) == 100 and len(_tuples(np.vstack([first, second]))) == 600
        calls = [np.vstack([points_in_voxel(rng, v, 1) for v in vs])[rng.permutation(len(vs))] for vs in (first, second)]
        capacity, aim = 100000, 2048
    else:
        rng = np.random.RandomState(301)  # both cases: the same two calls
        tail = lat[_inc_slots(1024)(lat) >= 1024 - INC_TAIL]
        tail = tail[rng.permutation(len(tail))[:60]]
        first, new = tail[:40], tail[40:]
        c1 = np.vstack([points_in_voxel(rng, v, 1 + i % 6) for i, v in enumerate(first)])
        again = first[rng.permutation(40)[:10]]
        c2 = np.vstack([points_in_voxel(rng, v, 1 + i % 3) for i, v in enumerate(again)] + [points_in_voxel(rng, v, 1 + i % 6) for i, v in enumerate(new)])
        calls = [c1[rng.permutation(len(c1))], c2[rng.permutation(len(c2))]]
        capacity, aim = (100000, 1024) if name == "lookup_chain" else (50, 1024)
        if name == "evict_from_chain":
            live = lru_replay(lru_replay(OrderedDict(), calls[0], capacity), calls[1], capacity)
            gone = sorted(_tuples(first) - set(live))
            assert len(gone) == 40 + 20 - (capacity - 1)
            back = np.array(gone[:5], dtype=np.int64)
            calls.append(np.vstack([points_in_voxel(rng, v, 2) for v in back]))
    calls = [np.ascontiguousarray(c, dtype=np.float32) for c in calls]
    live, lives, caps, points, cap, pts = OrderedDict(), [], [], [], 0, {}
    for c in calls:
        lru_replay(live, c, capacity)
        vox = voxels_of(c)
        for v in _tuples(vox):
            pts[v] = c[(vox == np.array(v)).all(axis=1)]  # a touched voxel's statistics are recomputed from this call's points alone
        pts = {v: p for v, p in pts.items() if v in live}
        cap = inc_capacity(len(live), cap)
        lives.append(np.array(sorted(live), dtype=np.int64))
        caps.append(cap)
        points.append(dict(pts))
    final = lives[-1]
    qrng = np.random.RandomState(9)
    occ, _ = probe_sim(_inc_slots(caps[-1])(final), caps[-1])
    inside = np.zeros(caps[-1], bool)
    inside[wrap_run(occ)] = True
    in_run = final[inside[_inc_slots(caps[-1])(final)]]
    others = final[~inside[_inc_slots(caps[-1])(final)]]
    asked = _tuples(np.concatenate([in_run[:80], others[qrng.permutation(len(others))[:40]]]))

    def near_mean(v):
        """Two points within 3 cm of the voxel's mean: single-point voxels carry info = 100·I and two-point voxels a rank-one covariance,
        so only a nearby query has a residual of ordinary size. Voxels that are not asked get no point."""
        if tuple(v.tolist()) not in asked:
            return np.zeros((0, 3), np.float32)
        m = points[-1][tuple(v.tolist())].astype(np.float64).mean(axis=0)
        p = np.clip(m + qrng.uniform(-0.03, 0.03, (2, 3)), v + 0.01, v + 0.99).astype(np.float32)
        assert (np.trunc(p.astype(np.float64)) == v).all()
        return p

    evicted = sorted(_tuples(np.vstack([voxels_of(c) for c in calls])) - _tuples(final))
    q = build_queries(qrng, final, _inc_slots(caps[-1]), caps[-1], near_mean, dropped=np.array(evicted[:4], dtype=np.int64).reshape(-1, 3))
    return dict(capacity=capacity, calls=calls, live=lives, caps=caps, points=points, queries=q, aim=aim)


# ---------------------------------------------------------------------------------------------- the oracle's side (handed in by the tests)
def oracle_direct(locref, cloud, nearby=1):
    ndt = locref.Ndt(method=1, nearby_type=nearby, res_outlier_th=RES_TH, min_pts_in_voxel=MIN_PTS)
    ndt.set_target(cloud)
    return ndt


def oracle_inc(locref, case, calls=None):
    """The oracle's incremental matcher after the first `calls` calls of the case (all of them by default)."""
    ndt = locref.Ndt(method=2, nearby_type=1, res_outlier_th=RES_TH, capacity=case["capacity"])
    for c in case["calls"][:calls]:
        ndt.set_target(c)
    return ndt


def restate(ref, ndt, pts, pose, nearby=1, weighted=False):
    """ndt_hb_ref.per_point of `pts` at `pose` against the oracle's dumped table, under the designed cases' gate."""
    keys, mu, info = ndt.dump()
    return ref.per_point(ref.Table(keys, mu, info), pts, pose, voxel_size=1.0, n_nearby=7 if nearby == 1 else 1, res_outlier_th=RES_TH, weighted=weighted)


def accepted_pairs(method, H, eff):
    """The exact witness of one evaluation's hits (ndt_hb_cases.accepted_pairs): direct NDT H[3,3] = H[4,4] = H[5,5], an integer held
    exactly in FP64; incremental NDT effective_num."""
    if method == 2:
        return int(eff)
    assert H[3, 3] == H[4, 4] == H[5, 5] and H[3, 3] == int(H[3, 3]), (H[3, 3], H[4, 4], H[5, 5])
    return int(H[3, 3])
