"""The NDT voxel records per voxel against a 60-digit reference (tests/ndt_voxel_ref.py) on designed voxels (tests/ndt_voxel_cases.py;
their conditions and the units are asserted on the CPU by tests/test_ndt_voxel_ref.py): ndt_voxel_record (csrc/ndt_ingest.hpp; the
direct table and the voxel set: S/(n-1), one-sided Jacobi with FMA and v_rsq_f64, the 1e-3·lam0 clamp, info = V diag(1/lam') U^T) and
inc_stats_kernel (csrc/ndt_inc.hip: info = (S + 1e-3 I)^-1 by cofactors). The oracle runs the same algorithms, so a comparison with it
cannot see a flaw of the algorithm; the reference is mp.eigsy and an mp inverse.

What is compared, and how:
  keys, counts     the dump holds exactly the designed voxels (min_pts_in_voxel 3 and 1; two incremental calls; voxel size 1 and 30);
  mu               the oracle's bits (direct; incremental to 1e-9 as in test_gpu_ndt_ingest_shapes.py) and within (n + 1)·u·max|p| of the
                   reference — a sequential double sum of n float32 values and one division;
  full rank        E/(u·kappa) <= 8 units of the case's group (ndt_voxel_cases.group_of, UNIT); E = max|info - ref|/max|ref|, u = 2^-53;
                   no full-rank case is excluded; the asymmetry max|info - info^T|/max|info| of the direct records to the same bar;
  coplanar         within the bar, at kappa_c = 1000, of T0 + T1 + T2 or T0 + T1 - T2 (T_k the reference's rank-one terms); which one is
                   printed and counted, the agreement with the oracle's choice is counted and not required;
  rank 1           (exactly collinear; two and three points) info·v0 = v0/lam0 and v0^T·info = v0^T/lam0 within the bar, every singular
                   value <= 1000/lam0·(1 + bar·u·1000), every entry finite;
  coincident       the record is not finite, a query inside the voxel is refused by the isnan(res) gate of ndt_hb (accepted pairs) and
                   leaves H and B of a scan it is added to unchanged, bit for bit;
  determinism      two ingests give the same bytes; the voxel set's records are the single-target build's, byte for byte.

The units (ndt_voxel_cases.UNIT, the oracle's own worst E/(u·kappa) per group, measured by test_ndt_voxel_ref.py) and what the MI355X
gave (every test prints its figures next to its bars):
    group         kappa                  unit   set by                                          device's worst
    direct        kappa_c                3.1    line 1e-02 at 100000 m (E 1.7e-14, kappa_c 49)  2.95
    direct line   lam0/lam1              1      line 4.22e-07 #0 (0.242; lam1/lam0 5.4e-11)     0.234
    direct long   kappa_c                360    n=4096 blob (the sums' own n·u)                 357.4
    inc           kappa_i                1.71   line 1e-05 at 500 m                             1.704
    inc line      kappa_i                970    line 0.003 #0, voxel size 30 (kappa_i 2.0e4)    966.4
    inc long      kappa_i                53     n=1024 blob                                     52.98
mu at most 0.12 of its bound; asymmetry of the direct info 1.6 u·kappa (the oracle's 2.2); all 12 coplanar voxels take +T2 on the
device and in the oracle (E/(u·1000) <= 0.01); two-dimensional null spaces: |info·v0 - v0/lam0|·lam0 <= 1.1e-13 (bar 2.75e-12), singular
values 1000/lam0·(1 ± 8e-16). Before the noise-column rule of csrc/ndt_ingest.hpp (kNdtNoiseRatio) the device's record of `collinear
n=7` had a singular value of 1.414·1000/lam0 and four of the twelve coplanar voxels took -T2. DESIGN.md §27 has the case table and the
mutation checks."""
import numpy as np
import pytest

import ndt_voxel_cases as vc
import ndt_voxel_ref as ref
from test_gpu_ndt_tables import _dump_bytes, _start_inc

pytestmark = pytest.mark.gpu

DIRECT = ("main", "tiny")
RES_TH = 1.0e6  # every residual that is a number is accepted: the accepted pairs of a scan count its voxels that have one


def _opts(api, t, **kw):
    if t["method"] == 1:
        return api.ndt_opts(voxel_size=t["voxel_size"], min_pts_in_voxel=t["min_pts"], **kw)
    return api.ndt_opts(method=api.INCREMENTAL_NDT, voxel_size=t["voxel_size"], capacity=100000, **kw)


def _ingest(gpu_ctx, api, t, **kw):
    if t["method"] == 2:
        _start_inc(gpu_ctx, api)
    counts = []
    for cloud in t["calls"]:
        gpu_ctx.ndt_set_target(cloud, _opts(api, t, **kw))
        counts.append(gpu_ctx.ndt_target_info()["num_voxels"])
    return counts


@pytest.fixture(scope="module")
def dumps(gpu_ctx, api, locref):
    """target → dict(gpu (keys, mu, info), oracle (keys, mu, info), counts, oracle_counts, figs, ofigs), each target ingested once."""
    cache = {}

    def get(name):
        if name not in cache:
            t, refs = vc.target(name), vc.reference(name)
            counts = _ingest(gpu_ctx, api, t)
            g = gpu_ctx.ndt_dump()
            ocounts = [vc.oracle_target(locref, t, calls=i + 1).num_voxels() for i in range(len(t["calls"]))]
            o = vc.oracle_target(locref, t).dump()
            cache[name] = dict(gpu=g, oracle=o, counts=counts, oracle_counts=ocounts,
                               figs=vc.record_figures(t, refs, vc.by_key(t, g[0]), g[1], g[2]),
                               ofigs=vc.record_figures(t, refs, vc.by_key(t, o[0]), o[1], o[2]))
        return cache[name]

    return get


# ---------------------------------------------------------------------------------------------- keys, counts, mu
@pytest.mark.parametrize("name", vc.TARGETS)
def test_keys_counts_and_means(dumps, name):
    t, d = vc.target(name), dumps(name)
    (kg, mug, _), (ko, muo, _) = d["gpu"], d["oracle"]
    assert d["counts"] == d["oracle_counts"] and d["counts"][-1] == len(t["cases"]) == len(kg) == len(ko)
    rg, ro = vc.by_key(t, kg), vc.by_key(t, ko)  # asserts that the dump's voxels are the cases' voxels, each once
    ig, io = np.array([rg[n] for n in t["cases"]]), np.array([ro[n] for n in t["cases"]])
    differ = int((mug[ig].view(np.uint64) != muo[io].view(np.uint64)).any(axis=1).sum())
    worst = max((f["mu_err"] / f["mu_bound"]).max() for f in d["figs"].values())
    print("%s: %d voxels; mu differs from the oracle's bits in %d of them; worst |mu - mu_ref| / ((n + 1) u max|p|) = %.3f (bar 1)" % (name, len(kg), differ, worst))
    if t["method"] == 1:
        assert differ == 0
    else:
        np.testing.assert_allclose(mug[ig], muo[io], rtol=0, atol=1e-9)
    for cname, f in d["figs"].items():
        assert (f["mu_err"] <= f["mu_bound"]).all(), (name, cname, f["mu_err"], f["mu_bound"])


# ---------------------------------------------------------------------------------------------- full-rank records
@pytest.mark.parametrize("name", vc.TARGETS)
def test_records_against_the_reference(dumps, name):
    """E/(u kappa) of every case that has a reference record — for a direct target the full-rank cases, for an incremental one all —
    against 8 units of its group; nothing is excluded."""
    t, d = vc.target(name), dumps(name)
    figs, ofigs = d["figs"], d["ofigs"]
    held = [n for n, f in figs.items() if f["group"] is not None]
    assert len(held) == sum(r["class"] == "full" for r in vc.reference(name).values()) if t["method"] == 1 else len(held) == len(t["cases"])
    ow = vc.worst_by(ofigs)
    for family, (w, who) in vc.worst_by(figs).items():
        print("%s, %-14s worst E/(u kappa) %9.3f (%s; %s, kappa %.4g) — the oracle's worst there %9.3f" % (name, family, w, who, figs[who]["group"], figs[who]["kappa"], ow[family][0]))
    og = vc.worst_by(ofigs, by="group")
    for group, (w, who) in vc.worst_by(figs, by="group").items():
        print("%s, group %-12s worst %9.3f = %.2f units (%s); bar %.1f units of %.4g; the oracle's worst %9.3f" % (name, group, w, w / vc.UNIT[group], who, vc.BAR_FACTOR, vc.UNIT[group], og[group][0]))
    bad = [(n, figs[n]["group"], figs[n]["fig"]) for n in held if not figs[n]["fig"] <= vc.BAR_FACTOR * vc.UNIT[figs[n]["group"]]]
    assert not bad, (name, bad[:8])
    if t["method"] == 1:
        asym = {n: figs[n]["asym"] / (ref.U * figs[n]["kappa"]) for n in held}
        who = max(asym, key=asym.get)
        oasym = {n: ofigs[n]["asym"] / (ref.U * ofigs[n]["kappa"]) for n in held}
        owho = max(oasym, key=oasym.get)
        print("%s: worst asymmetry of the direct info %.3e = %.3f u kappa (%s, %s); the oracle's %.3e = %.3f u kappa (%s)" % (
            name, figs[who]["asym"], asym[who], who, figs[who]["group"], ofigs[owho]["asym"], oasym[owho], owho))
        bad = [(n, figs[n]["group"], asym[n]) for n in held if not asym[n] <= vc.BAR_FACTOR * vc.UNIT[figs[n]["group"]]]
        assert not bad, (name, bad[:8])


# ---------------------------------------------------------------------------------------------- rank-deficient direct records
def test_rank_deficient_direct_records(dumps):
    bar = vc.BAR_FACTOR * vc.UNIT["direct"]
    signs, agree, n_def = [], 0, 0
    for name in DIRECT:
        t, refs, d = vc.target(name), vc.reference(name), dumps(name)
        rg, ro = vc.by_key(t, d["gpu"][0]), vc.by_key(t, d["oracle"][0])
        for cname, c in t["cases"].items():
            if refs[cname]["class"] == "full":
                continue
            n_def += 1
            v = vc.deficient_verdict(c, refs[cname], d["gpu"][2][rg[cname]], bar)
            vo = vc.deficient_verdict(c, refs[cname], d["oracle"][2][ro[cname]], bar)
            print("%s / %-24s %-10s %s" % (name, cname, v["kind"], v["text"]))
            assert v["ok"], (name, cname, v["text"])
            if v["kind"] == "coplanar":
                signs.append(v["sign"])
                agree += v["sign"] == vo["sign"]
    print("coplanar voxels: %d of %d take +T2, %d take -T2; %d agree with the oracle's choice (not required)" % (signs.count(1), len(signs), signs.count(-1), agree))
    assert len(signs) == len(vc.COPLANAR_N) and n_def == 24


def test_coincident_voxel_refuses_its_queries(gpu_ctx, api):
    t, refs = vc.target("main"), vc.reference("main")
    _ingest(gpu_ctx, api, t, res_outlier_th=RES_TH)
    keys, _, info = gpu_ctx.ndt_dump()
    c = t["cases"]["coincident"]
    assert not np.isfinite(info[vc.by_key(t, keys)["coincident"]]).any()
    inside = (c["points"][:1].astype(np.float64) + 0.01).astype(np.float32)
    nowhere = np.array([[200.5, 200.5, 200.5]], np.float32)  # an empty voxel with empty neighbours
    assert tuple(ref.keys_of(inside)[0]) == c["key"] and (ref.keys_of(nowhere)[0] == 200).all()
    scan = np.vstack([cc["design"][:1] + np.float32(0.001) for n, cc in t["cases"].items() if refs[n]["class"] == "full" and cc["family"] != "placement"][:30])
    assert (ref.keys_of(scan) == ref.keys_of(scan - np.float32(0.001))).all()
    pose = np.array([0, 0, 0, 1.0, 0, 0, 0])
    ok, H, B, eff = gpu_ctx.ndt_hb(inside, pose)
    print("one query inside the coincident voxel: accepted pairs %g, effective_num %d, max|H| %g, max|B| %g" % (H[3, 3], eff, np.abs(H).max(), np.abs(B).max()))
    assert np.isfinite(H).all() and np.isfinite(B).all() and (H == 0).all() and (B == 0).all() and eff == 1 and not ok
    with_q = gpu_ctx.ndt_hb(np.vstack([scan, inside]), pose)
    without = gpu_ctx.ndt_hb(np.vstack([scan, nowhere]), pose)
    print("a scan of %d points plus that query: accepted pairs %g; plus a point in an empty voxel instead: %g" % (len(scan), with_q[1][3, 3], without[1][3, 3]))
    assert with_q[1][3, 3] == without[1][3, 3] == len(scan)  # every other point finds its one voxel
    assert with_q[1].tobytes() == without[1].tobytes() and with_q[2].tobytes() == without[2].tobytes() and with_q[3] == without[3] and with_q[0] == without[0]
    assert np.isfinite(with_q[1]).all() and np.isfinite(with_q[2]).all()


# ---------------------------------------------------------------------------------------------- determinism, the voxel set
@pytest.mark.parametrize("name", vc.TARGETS)
def test_two_ingests_give_the_same_bytes(gpu_ctx, api, dumps, name):
    first = _dump_bytes(dumps(name)["gpu"])
    _ingest(gpu_ctx, api, vc.target(name))
    assert _dump_bytes(gpu_ctx.ndt_dump()) == first


def test_voxel_set_records_equal_the_single_target_build(gpu_ctx, api):
    """`main` and `tiny` as the two targets of one voxel set (min_pts_in_voxel 1 for both: every voxel of `main` has four points or
    more, so it keeps the same voxels) against each cloud ingested alone with the same options. A set's keys span ±2^15 voxels, so
    `main` goes in without its four cases 100 000 m out."""
    clouds = [vc.target(n)["calls"][0] for n in DIRECT]
    clouds = [np.ascontiguousarray(c[(np.abs(ref.keys_of(c)) < (1 << 15)).all(axis=1)]) for c in clouds]
    want = [len(vc.target("main")["cases"]) - 4, len(vc.target("tiny")["cases"])]
    assert len(clouds[0]) == len(vc.target("main")["calls"][0]) - 4 * vc.N_PTS
    opts = api.ndt_opts(voxel_size=1.0, min_pts_in_voxel=1)
    ctx = api.Context(0)
    try:
        ctx.ndt_set_target_set(clouds, opts)
        assert ctx.ndt_set_info()["voxels"] == want
        for i, name in enumerate(DIRECT):
            gpu_ctx.ndt_set_target(clouds[i], opts)
            single, of_set = gpu_ctx.ndt_dump(), ctx.ndt_set_dump(i)
            assert len(single[0]) == len(of_set[0]) == want[i]
            assert _dump_bytes(single) == _dump_bytes(of_set), name
            print("voxel set target %d (%s): %d records byte-identical to the single-target build" % (i, name, len(single[0])))
    finally:
        ctx.close()
