"""CPU side of the NDT voxel-record tests: the 60-digit reference (tests/ndt_voxel_ref.py) against long-double numpy and against voxels
that can be computed by hand; the conditions of the designed cases (tests/ndt_voxel_cases.py) from the reference alone; and the ORACLE
on the same cases, which is where the units of tests/test_gpu_ndt_voxels.py are measured (run with -s to see the figures)."""
import numpy as np
import pytest
from mpmath import mp, mpf

import ndt_voxel_cases as vc
import ndt_voxel_ref as ref

LD = np.longdouble
DIRECT = ("main", "tiny")
INC = ("inc1", "inc30")


# ---------------------------------------------------------------------------------------------- the reference itself
def _longdouble_records(p):
    """(direct, incremental) record of float32 points with the covariance formed in long double and numpy's eigh / inv in double."""
    q = np.asarray(p, dtype=np.float32).astype(LD)
    d = q - q.sum(axis=0) / LD(len(q))
    cov = (d.T @ d) / LD(len(q) - 1)
    w, v = np.linalg.eigh(cov.astype(np.float64))
    w, v = w[::-1].astype(LD), v[:, ::-1].astype(LD)
    lam = np.maximum(w, LD(1e-3) * w[0])
    direct = (v / lam) @ v.T
    inc = np.linalg.inv((cov + LD(1e-3) * np.eye(3, dtype=LD)).astype(np.float64))
    return direct.astype(np.float64), inc


def test_reference_matches_longdouble_eigh_on_well_conditioned_voxels():
    worst = (0.0, None, 0.0, None)
    n = 0
    for name in vc.TARGETS:
        refs = vc.reference(name)
        for cname, c in vc.target(name)["cases"].items():
            r = refs[cname]
            if r["class"] != "full" or float(r["kappa_c"]) > 2.0:
                continue
            n += 1
            direct, inc = _longdouble_records(c["points"])
            ed, ei = ref.rel_err(direct, r["direct"]), ref.rel_err(inc, r["inc"])
            if ed > worst[0]:
                worst = (ed, cname) + worst[2:]
            if float(r["kappa_i"]) <= 2.0 and ei > worst[2]:
                worst = worst[:2] + (ei, cname)
    print("reference vs long-double numpy on %d voxels with kappa_c <= 2: direct %.2e (%s), incremental %.2e (%s); bar 1e-15" % ((n,) + worst))
    assert n >= 6 and worst[0] <= 1e-15 and worst[2] <= 1e-15


def test_reference_inverse_and_eigenpairs_are_consistent_at_60_digits():
    for name in ("main", "inc30"):
        for cname, r in vc.reference(name).items():
            if r["n"] == 1:
                continue
            with mp.workdps(ref.DPS):
                res = r["inc"] * (r["cov"] + mp.eye(3) * ref.INC_EPS) - mp.eye(3)
                assert max(abs(x) for x in res) < mpf(10) ** -50, cname
                assert r["lam"][0] >= r["lam"][1] >= r["lam"][2] >= 0
                if r["lam"][0] == 0:
                    continue
                scale = r["lam"][0]
                for k in range(3):
                    v = mp.matrix(r["vec"][k])
                    assert max(abs(x) for x in r["cov"] * v - v * r["lam"][k]) < scale * mpf(10) ** -50, (cname, k)
                    assert abs((v.T * v)[0] - 1) < mpf(10) ** -50


def _corners(c, h):
    return vc.cube(c, h, 0)


def test_reference_on_voxels_computed_by_hand():
    # the 8 corners of a box with half-widths (a, b, c): mu = centre, S = 8/7·diag(a², b², c²)
    a, b, c = 0.25, 0.125, 0.0625
    r = ref.record(_corners((1.5, 3.5, 5.5), (a, b, c)))
    var = [8.0 / 7.0 * x * x for x in (a, b, c)]
    assert [float(x) for x in r["mu"]] == [1.5, 3.5, 5.5]
    assert np.allclose(ref.to_float(r["cov"]), np.diag(var), rtol=0, atol=1e-50)
    assert np.allclose([float(x) for x in r["lam"]], var, rtol=1e-50)
    assert np.allclose(ref.to_float(r["direct"]), np.diag([1 / v for v in var]), rtol=1e-15, atol=1e-13)  # lam2/lam0 = 1/16: no clamp
    assert np.allclose(ref.to_float(r["inc"]), np.diag([1 / (v + 1e-3) for v in var]), rtol=1e-15, atol=1e-13)
    assert abs(float(r["kappa_c"]) - 16.0) < 1e-12 and abs(float(r["kappa_i"]) - (var[0] + 1e-3) / (var[2] + 1e-3)) < 1e-12
    # a flat box: lam2/lam0 = 2^-12 < 1e-3, lam1/lam0 = 1/4: only the last value is clamped, to 1e-3·lam0
    r = ref.record(_corners((1.5, 3.5, 5.5), (0.25, 0.125, 0.25 / 64)))
    l0 = 8.0 / 7.0 * 0.0625
    assert np.allclose(ref.to_float(r["direct"]), np.diag([1 / l0, 4 / l0, 1000 / l0]), rtol=1e-15, atol=1e-12)
    assert float(r["kappa_c"]) == 1000.0 and ref.rank_class(r) == "full"
    # a needle: both small values clamped
    r = ref.record(_corners((1.5, 3.5, 5.5), (0.25, 0.25 / 64, 0.25 / 128)))
    assert np.allclose(ref.to_float(r["direct"]), np.diag([1 / l0, 1000 / l0, 1000 / l0]), rtol=1e-15, atol=1e-12)
    # the cube with two centre copies: S = 8 h²/9·I, whatever the eigenvectors
    r = ref.record(vc.cube((1.5, 1.5, 1.5), 0.25, 2))
    assert np.allclose(ref.to_float(r["direct"]), np.eye(3) * 9 / (8 * 0.0625), rtol=1e-15, atol=1e-13) and float(r["kappa_c"]) == 1.0
    # one point, two points, coincident points
    r = ref.record(np.array([[1.25, 2.5, 3.75]], np.float32))
    assert [float(x) for x in r["mu"]] == [1.25, 2.5, 3.75] and np.array_equal(ref.to_float(r["inc"]), 100 * np.eye(3)) and ref.rank_class(r) == "single"
    r = ref.record(np.array([[1.25, 2.5, 3.5], [1.75, 2.5, 3.5]], np.float32))  # S = diag(0.125, 0, 0)
    assert ref.rank_class(r) == "deficient" and float(r["lam"][0]) == 0.125 and float(r["lam"][1]) == 0.0
    assert np.allclose(ref.to_float(r["inc"]), np.diag([1 / 0.126, 1000, 1000]), rtol=1e-15)
    assert np.allclose(ref.to_float(r["terms"][0]), np.diag([8.0, 0, 0]), rtol=1e-15, atol=1e-50)
    r = ref.record(np.tile(np.array([[1.3, 2.6, 3.7]], np.float32), (6, 1)))
    assert ref.rank_class(r) == "coincident" and r["direct"] is None and np.allclose(ref.to_float(r["inc"]), 1000 * np.eye(3), rtol=1e-15)


def test_key_rule_truncates_toward_zero():
    p = np.array([[0.9, -0.9, 1.0], [-1.0, -1.5, 2.99], [29.9, 30.0, -30.1]], np.float32)
    assert ref.keys_of(p).tolist() == [[0, 0, 1], [-1, -1, 2], [29, 30, -30]]
    assert ref.keys_of(p, 30.0).tolist() == [[0, 0, 0], [0, 0, 0], [0, 1, -1]]


# ---------------------------------------------------------------------------------------------- the designed cases
@pytest.mark.parametrize("name", vc.TARGETS)
def test_case_conditions(name):
    """Every case lies in one voxel, no two cases share a voxel or a face, every voxel of the joined cloud belongs to a case, and no
    case falls between the two rank classes."""
    t, refs = vc.target(name), vc.reference(name)
    seen = {}
    keys = np.vstack([ref.keys_of(cloud, t["voxel_size"]) for cloud in t["calls"]])
    assert (np.abs(keys) < (1 << 20)).all()
    assert {tuple(k) for k in keys.tolist()} == {c["key"] for c in t["cases"].values()}  # a later call only returns to voxels or adds cases
    for cname, c in t["cases"].items():
        k = ref.keys_of(c["design"], t["voxel_size"])
        assert (k == k[0]).all(), (cname, "leaves its voxel")
        assert tuple(k[0].tolist()) == c["key"]
        assert len(c["points"]) == len(c["design"]) and np.array_equal(np.sort(c["points"], axis=0), np.sort(c["design"], axis=0)), cname
        assert c["key"] not in seen, (cname, seen.get(c["key"]), "share a voxel")
        seen[c["key"]] = cname
        assert refs[cname]["class"] != "band", (cname, float(refs[cname]["ratio"]), "between full rank and rank-deficient")
    for key, cname in seen.items():
        for ax in range(3):
            for d in (-1, 1):
                nb = list(key)
                nb[ax] += d
                assert tuple(nb) not in seen, (cname, seen.get(tuple(nb)), "share a face")
    classes = {}
    for r in refs.values():
        classes[r["class"]] = classes.get(r["class"], 0) + 1
    print("%s: %d cases, %d points in %d call(s); %s" % (name, len(t["cases"]), sum(len(c) for c in t["calls"]), len(t["calls"]), classes))
    if t["method"] == 1:  # the direct build keeps a voxel with MORE points than min_pts_in_voxel
        assert all(len(c["points"]) > t["min_pts"] for c in t["cases"].values())


def test_families_cover_what_they_are_for():
    t, refs = vc.target("main"), vc.reference("main")
    fam = lambda f: [(n, refs[n]) for n, c in t["cases"].items() if c["family"] == f]
    plane = [float(r["ratio"]) for _, r in fam("plane ladder")]
    assert min(plane) < 1e-11 and max(plane) > 0.1 and sum(1e-3 < x < 1e-1 for x in plane) >= 3 and sum(1e-5 < x < 1e-3 for x in plane) >= 3  # both sides of the clamp
    line1 = [float(r["lam"][1] / r["lam"][0]) for _, r in fam("line ladder")]
    assert min(line1) < 1e-11 and max(line1) > 0.1 and sum(1e-12 < x < 2e-10 for x in line1) >= 20  # the near-collinear peak's neighbourhood
    for n, r in fam("clamp edge"):
        k = 2 if "lam2" in n else 1
        x = float(r["lam"][k] / r["lam"][0]) / 1e-3 - 1.0
        assert abs(x) <= 1e-6 and (x > 0) == ("+5e-07" in n), (n, x)
        assert (float(r["lam"][1] / r["lam"][0]) > 0.1) if k == 2 else (float(r["ratio"]) < 1e-4)
    for n, r in fam("equal values"):
        assert float(r["lam"][1] / r["lam"][2]) - 1.0 < 1e-5, n  # tilted: equal to float32 rounding
        assert (float(r["lam"][0] / r["lam"][1]) - 1.0 < 1e-5) == n.startswith("cube") and (n.startswith("cube") or float(r["lam"][0] / r["lam"][1]) > 2)
    assert all(r["class"] == "deficient" and float(r["lam"][1] / r["lam"][0]) > 1e-2 for _, r in fam("coplanar")) and len(fam("coplanar")) == len(vc.COPLANAR_N)
    assert all(r["class"] == "deficient" and float(r["lam"][1] / r["lam"][0]) < 1e-20 for _, r in fam("rank 1"))
    assert sorted(len(t["cases"][n]["points"]) for n, _ in fam("counts")) == [4] * 4 + [5] * 4 + [1024] * 2 + [4096] * 2
    assert all(r["class"] == "full" for _, r in fam("counts") + fam("placement") + fam("clamp edge") + fam("equal values"))
    keys = np.array([t["cases"][n]["key"] for n, _ in fam("placement")])
    assert (keys.min(axis=1) >= 100000).sum() == 4 and (keys.max(axis=1) < 0).sum() == 4 and (keys == 0).any(axis=1).sum() == 4
    i1, i30 = vc.reference("inc1"), vc.reference("inc30")
    assert max(float(r["kappa_i"]) for r in i30.values()) > 2e4 and sum(r["class"] == "single" for r in i1.values()) >= 4
    assert sum(c["call"] == 1 for c in vc.target("inc1")["cases"].values()) == 11


# ---------------------------------------------------------------------------------------------- the oracle on the same cases
@pytest.fixture(scope="module")
def oracle_figures(locref):
    out = {}
    for name in vc.TARGETS:
        t = vc.target(name)
        ndt = vc.oracle_target(locref, t)
        keys, mu, info = ndt.dump()
        out[name] = (vc.record_figures(t, vc.reference(name), vc.by_key(t, keys), mu, info), keys, mu, info)
    return out


def _units(figs_of, names):
    """group → (worst figure, target, case) over the targets `names`."""
    worst = {}
    for name in names:
        for cname, f in figs_of[name][0].items():
            if f["fig"] is not None and f["fig"] > worst.get(f["group"], (-1.0,))[0]:
                worst[f["group"]] = (f["fig"], name, cname)
    return worst


def test_units_of_the_oracle(oracle_figures):
    """The oracle's worst E/(u kappa) per group of ndt_voxel_cases.group_of: the direct record over the full-rank cases of `main` and
    `tiny`, the incremental record over every case of `inc1` and `inc30`. vc.UNIT records them, never below 1."""
    worst = dict(_units(oracle_figures, DIRECT), **_units(oracle_figures, INC))
    assert sorted(worst) == sorted(vc.UNIT)
    for group in vc.UNIT:
        fig, name, cname = worst[group]
        r, f = vc.reference(name)[cname], oracle_figures[name][0][cname]
        print("unit %-12s %8.3f (E = %.3e) set by %s / %s (n %d, lam1/lam0 %.3e, lam2/lam0 %.3e, kappa_c %.4g, kappa_i %.4g, kappa used %.4g); recorded %.4g" % (
            group, fig, f["E"], name, cname, r["n"], float(r["lam"][1] / r["lam"][0]), float(r["ratio"]), float(r["kappa_c"]), float(r["kappa_i"]), f["kappa"], vc.UNIT[group]))
    for name in vc.TARGETS:
        for family, (w, who) in vc.worst_by(oracle_figures[name][0]).items():
            print("    oracle, %-5s %-14s worst %8.3f  (%s, %s)" % (name, family, w, who, oracle_figures[name][0][who]["group"]))
    for group in vc.UNIT:
        fig = worst[group][0]
        assert np.isfinite(fig) and max(fig, 1.0) <= vc.UNIT[group] <= 1.1 * max(fig, 1.0), (group, fig, vc.UNIT[group])
    # the near-collinear voxels in the measure that does not see them: E/(u kappa_c), kappa_c = 1000
    line = {n: f["E"] / (ref.U * 1000.0) for n, f in oracle_figures["main"][0].items() if f["group"] == "direct line"}
    who = max(line, key=line.get)
    print("    oracle, near-collinear voxels in E/(u·1000): worst %.3e (%s, E = %.3e)" % (line[who], who, oracle_figures["main"][0][who]["E"]))


def test_oracle_mu_within_the_derived_bound_and_asymmetry(oracle_figures):
    for name in vc.TARGETS:
        figs = oracle_figures[name][0]
        worst = max((f["mu_err"] / f["mu_bound"]).max() for f in figs.values())
        print("%s: oracle's worst |mu - mu_ref| / ((n + 1) u max|p|) = %.3f" % (name, worst))
        assert worst <= 1.0
    for name in DIRECT:
        full = {n: f for n, f in oracle_figures[name][0].items() if f["group"] is not None}
        asym = {n: f["asym"] / (ref.U * f["kappa"]) / vc.UNIT[f["group"]] for n, f in full.items()}
        who = max(asym, key=asym.get)
        print("%s: oracle's worst asymmetry of the direct info %.3e = %.2f units of its group (%s, %s)" % (name, full[who]["asym"], asym[who], who, full[who]["group"]))
        assert asym[who] <= vc.BAR_FACTOR


def test_oracle_records_of_rank_deficient_voxels_obey_the_rules(oracle_figures):
    """The rules test_gpu_ndt_voxels.py holds the device to, on the reference side alone: coplanar voxels on one of two candidates,
    a null space of two dimensions without leakage into v0, coincident points not finite. Which sign each coplanar voxel takes is
    printed; the device's need not agree."""
    bar = vc.BAR_FACTOR * vc.UNIT["direct"]
    signs = []
    for name in DIRECT:
        t, refs = vc.target(name), vc.reference(name)
        figs, keys, mu, info = oracle_figures[name]
        rows = vc.by_key(t, keys)
        for cname, c in t["cases"].items():
            if refs[cname]["class"] == "full":
                continue
            v = vc.deficient_verdict(c, refs[cname], info[rows[cname]], bar)
            print("oracle, %s / %-24s %-10s %s" % (name, cname, v["kind"], v["text"]))
            assert v["ok"], (name, cname, v["text"])
            if v["kind"] == "coplanar":
                signs.append(v["sign"])
    print("oracle: %d of %d coplanar voxels take the minus sign" % (signs.count(-1), len(signs)))
    assert len(signs) == len(vc.COPLANAR_N)
