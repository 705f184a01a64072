"""tests/icp_hb_ref.py, the mpmath restatement the GPU tests of the ICP fit kernels compare per point — closed forms first, then its
sums over a scan against the oracle's locref.Icp.hb, then the oracle's own per-point error in units of u·κ: the units of
tests/test_gpu_icp_hb.py, recorded in icp_hb_cases.UNIT."""
import numpy as np
import pytest

import icp_hb_cases as cases
import icp_hb_ref as ref
import map_plane_ref
from test_gpu_parity import HB_RTOL, _hb_close

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
TINY = 1e-40  # the restatement carries 60 digits: a singular vector is exact to ~1e-58, never to the last digit


def _hat(q):
    return np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])


def _same(pp, J, e):
    """H, B of point 0 equal JᵀJ, −Jᵀe exactly: every number is a short dyadic fraction, so the FP64 products are exact and the
    restatement's hi part must round onto them (an exact zero comes out as 1e-58 or so)."""
    H, B = J.T @ J, -(J.T @ e)
    for got, lo, want in ((pp["H"][0], pp["H_lo"][0], H), (pp["B"][0], pp["B_lo"][0], B)):
        assert (np.abs(lo) <= TINY).all() and (np.abs(got - want) <= TINY).all()
        np.testing.assert_array_equal(got[want != 0], want[want != 0])


@pytest.fixture(scope="module")
def inputs(locref, small_world):
    return cases.input_sets(locref, small_world)


@pytest.fixture(scope="module")
def restated(locref, inputs):
    """(input set, method) → the restatement, once per module; map-plane with the oracle's table rows."""
    out = {}
    for name, inp in inputs.items():
        for method in cases.ORACLE_METHODS:
            out[name, method] = cases.restate(locref, inp, method)
        nn1 = cases.neighbours(locref, inp["tree"], inp["scan"], inp["pose"], cases.MAPPLANE, approximate=inp["approximate"])
        planes = cases.oracle_plane_rows(locref, inp["tree"], inp["map"], nn1[:, 0])
        out[name, "planes"] = planes
        out[name, cases.MAPPLANE] = cases.restate(locref, inp, cases.MAPPLANE, planes=planes)
    return out


# ---- closed forms of the restatement
def test_identity_pose_point_to_point_and_its_gate_at_equality():
    m = np.array([[2.5, 3.25, 4.75], [3.25, 3.5, 4.5], [np.nextafter(np.float32(3.25), np.float32(4)), 3.5, 4.5]], np.float32)
    q = np.array([2.25, 3.5, 4.5])
    s = q[None].astype(np.float32)
    pp = ref.per_point(ref.P2P, m, [[0]], s, IDENT)
    assert pp["fitted"].tolist() == [True] and pp["accepted"].tolist() == [True] and pp["kappa"].tolist() == [1.0]
    J = np.hstack([_hat(q) / 16, -np.eye(3)])
    _same(pp, J, m[0].astype(np.float64) - q)
    assert pp["gates"][0, 0] == 1 - 0.1875
    # e·e == max_nn_distance exactly is accepted (`dis2 > max_nn_distance` refuses), the next float above is refused
    at = ref.per_point(ref.P2P, m, [[1]], s, IDENT)
    assert at["accepted"].tolist() == [True] and at["gates"][0, 0] == 0 and ref.near_gate(at).tolist() == [True]
    _same(at, J, np.array([1.0, 0, 0]))
    above = ref.per_point(ref.P2P, m, [[2]], s, IDENT)
    assert above["accepted"].tolist() == [False] and above["fitted"].tolist() == [False] and 0 < above["gates"][0, 0] < 1e-6
    assert not above["H"].any() and not above["B"].any() and ref.near_gate(above, 1e-9).tolist() == [False]
    assert ref.per_point(ref.P2P, m, [[0]], s, IDENT, max_nn_distance=0.1875)["accepted"].tolist() == [True]
    assert ref.per_point(ref.P2P, m, [[0]], s, IDENT, max_nn_distance=np.nextafter(0.1875, 0))["accepted"].tolist() == [False]
    # no neighbour, and the finite-point rule
    bad = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [1.0, 2.0, 3.0]], np.float32)
    none = ref.per_point(ref.P2P, m, [[0], [0], [-1]], bad, IDENT)
    assert not none["fitted"].any() and not none["H"].any() and np.isinf(none["gates"]).all()


PLANE_NB = np.array([[0, 0, -1], [1, 0, -2], [0, 1, -2], [-1, 0.5, -0.5], [0.5, -1, -0.5]], np.float32)  # on x + y + z + 1 = 0: n4 = ±(½, ½, ½, ½)


def test_identity_pose_point_to_plane_and_the_table_look_up():
    q = np.array([0.25, 0.5, -1.625])
    s = q[None].astype(np.float32)
    pp = ref.per_point(ref.P2PLANE, PLANE_NB, [[0, 1, 2, 3, 4]], s, IDENT)
    assert pp["fitted"].tolist() == [True] and pp["accepted"].tolist() == [True] and not pp["rank_deficient"].any()
    assert ref.vector_errors(np.full((1, 4), 0.5), pp["vec"], pp["vec_lo"])[0] <= TINY
    n3 = np.array([0.5, 0.5, 0.5])  # a unit 4-vector: |n3| is not 1
    J = np.hstack([-(n3 @ _hat(q)), n3])[None]
    dis = n3 @ q + 0.5
    assert dis == 0.0625
    _same(pp, J, np.array([dis]))
    assert np.isfinite(pp["kappa"][0]) and pp["kappa"][0] > 1
    assert np.allclose(pp["gates"][0], [1, 1, 1, 1, 1, 1 - 0.625], atol=1e-30, rtol=1e-15)  # five squared errors of 0, |dis| = 0.0625 of 0.1
    # the residual gate: |dis| > max_plane_distance refuses, and the point still counts as fitted (effective_num++ comes first)
    far = ref.per_point(ref.P2PLANE, PLANE_NB, [[0, 1, 2, 3, 4]], s, IDENT, max_plane_distance=0.0625 * (1 - 2.0 ** -50))
    assert far["fitted"].tolist() == [True] and far["accepted"].tolist() == [False] and not far["H"].any()
    # the fit gate: a fifth point whose squared error passes 1e-2
    off = PLANE_NB.copy()
    off[4, 2] += 1.0
    bent = ref.per_point(ref.P2PLANE, off, [[0, 1, 2, 3, 4]], s, IDENT)
    assert bent["fitted"].tolist() == [False] and bent["accepted"].tolist() == [False]
    # the same row from a table entry; an invalid row contributes nothing, not even to effective_num
    table = (np.array([[-0.5, -0.5, -0.5, -0.5], [0.5, 0.5, 0.5, 0.5]]), np.array([True, False]))
    mp_ = ref.per_point(ref.MAPPLANE, PLANE_NB, [[0]], s, IDENT, planes=table)
    assert mp_["fitted"].tolist() == [True] and mp_["accepted"].tolist() == [True] and mp_["kappa"].tolist() == [1.0]
    _same(mp_, J, np.array([dis]))  # the sign of n4 cancels
    inv = ref.per_point(ref.MAPPLANE, PLANE_NB, [[1]], s, IDENT, planes=table)
    assert not inv["fitted"].any() and not inv["H"].any()


def test_identity_pose_point_to_line():
    m = np.array([[-1, 2, 3], [0, 2, 3], [1, 2, 3], [2, 2, 3], [3, 2, 3]], np.float32)  # p0 = (1, 2, 3), d = ±(1, 0, 0)
    q = np.array([0.5, 2.25, 3.125])
    s = q[None].astype(np.float32)
    pp = ref.per_point(ref.P2LINE, m, [[0, 1, 2, 3, 4]], s, IDENT)
    assert pp["fitted"].tolist() == [True] and pp["accepted"].tolist() == [True] and pp["kappa"].tolist() == [1.0]  # σ2 = 0
    assert ref.vector_errors(np.array([[1.0, 0, 0]]), pp["vec"][:, :3], pp["vec_lo"][:, :3])[0] <= TINY
    d = np.array([1.0, 0, 0])
    e = np.cross(d, q - [1, 2, 3])
    J = np.hstack([-_hat(d) @ _hat(q), _hat(d)])
    _same(pp, J, e)
    # |e|² = 0.078125: the residual gate compares the NORM, the fit gate the SQUARED distances of the neighbours (all 0 here)
    assert ref.per_point(ref.P2LINE, m, [[0, 1, 2, 3, 4]], s, IDENT, max_line_distance=0.25)["accepted"].tolist() == [False]
    assert ref.per_point(ref.P2LINE, m, [[0, 1, 2, 3, 4]], s, IDENT, max_line_distance=0.28)["accepted"].tolist() == [True]
    bent = m.copy()
    bent[2, 1] += 1.0  # p0 = (1, 2.2, 3), d stays ±x: that neighbour lies 0.8 from the line, squared 0.64 > 0.5
    r = ref.per_point(ref.P2LINE, bent, [[0, 1, 2, 3, 4]], s, IDENT)
    assert r["fitted"].tolist() == [False] and (r["gates"][0, :5] < np.inf).all() and r["gates"][0, 5] == np.inf
    assert ref.per_point(ref.P2LINE, bent, [[0, 1, 2, 3, 4]], s, IDENT, max_line_distance=0.7)["fitted"].tolist() == [True]


def test_rank_and_conditioning_of_designed_neighbourhoods():
    dm, kind = cases.designed_map()
    assert len(dm) == 5 * cases.PER_KIND * len(cases.KINDS) and np.bincount(kind).tolist() == [cases.PER_KIND] * len(cases.KINDS)
    cen = dm.reshape(-1, 5, 3).mean(axis=1).astype(np.float64)
    d = np.linalg.norm(cen[:, None] - cen[None], axis=2) + 1e9 * np.eye(len(cen))
    assert d.min() >= 6.0
    for name, deficient in (("coplanar_exact", False), ("collinear_exact", True)):
        c = int(np.flatnonzero(kind == cases.KINDS.index(name))[0])
        t = ref.plane_table(dm, [np.arange(5 * c, 5 * c + 5)])
        assert t["rank_deficient"].tolist() == [deficient] and t["valid"].tolist() == [True]
        assert (t["kappa"][0] > cases.KAPPA_MAX) == deficient  # σ3 = σ4 = 0 but for the 60th digit
    far = np.linalg.norm(cen[kind == cases.KINDS.index("far_300_500m")], axis=1)
    assert far.min() >= 299 and far.max() <= 501
    z = dm.reshape(-1, 5, 3)[kind == cases.KINDS.index("coplanar_exact")][:, :, 2]
    assert (z == z[:, :1]).all()


def test_rotation_is_the_oracles(locref):
    pose = np.array([0.02, -0.03, 0.3, 0.0, 1.5, -2.5, 0.25])
    pose[3] = np.sqrt(1 - (pose[:3] ** 2).sum())
    pts = np.array([[1.0, 2.0, 3.0], [-30.5, 12.25, 0.75]])
    want = locref.transform_points(pose, pts)
    R = np.array([[float(v) for v in row] for row in ref.rotation(pose)])
    assert np.abs(pts @ R.T + pose[4:] - want).max() <= 1e-14


# ---- the restatement summed over a scan is the oracle's evaluation
@pytest.mark.parametrize("method", cases.ORACLE_METHODS)
def test_restatement_summed_equals_oracle_hb(locref, small_world, inputs, method):
    """scan2k: the 10 000-point restatement of the plane method costs about a minute."""
    scan, pose, m = small_world["scan2k"], small_world["init_pose"], small_world["map"]
    icp = locref.Icp(method=method)
    icp.set_target(m)
    ok, Ho, Bo, eff = icp.hb(scan, pose)
    nn = cases.neighbours(locref, inputs["init_pose"]["tree"], scan, pose, method)
    pp = ref.per_point(method, m, nn, scan, pose)
    Hr, Br, fitted, accepted = ref.totals(pp)
    scale = np.abs(Ho).max()
    print("%s: |H-H_ref|/max|H| = %.2e (bar %.0e), |B-B_ref| = %.2e (|B| %.2e), effective_num %d / %d, accepted %d of %d points"
          % (cases.NAMES[method], np.abs(Hr - Ho).max() / scale, HB_RTOL, np.abs(Br - Bo).max(), np.abs(Bo).max(), fitted, eff, accepted, len(scan)))
    _hb_close(Hr, Br, Ho, Bo)
    assert ok and accepted >= 1000
    assert not cases.excluded(pp).any()  # then the counts are exact on either side
    assert eff == fitted
    if method == cases.P2P:  # the −I3 block of every accepted point: a count, exact in FP64
        assert Ho[3, 3] == Ho[4, 4] == Ho[5, 5] == accepted
    # the accepted points one by one: a refused point leaves the oracle's H exactly zero
    refused = np.flatnonzero(pp["fitted"] & ~pp["accepted"])[:40]
    for i in np.concatenate([refused, np.flatnonzero(pp["accepted"])[:40]]):
        _, H1, _, eff1 = icp.hb(scan[i:i + 1], pose)
        assert bool(H1.any()) == bool(pp["accepted"][i]) and eff1 == int(pp["fitted"][i]), i


def _one_point_rows(hb_of, scan):
    rows = [hb_of(scan[i:i + 1]) for i in range(len(scan))]
    return np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.array([r[3] for r in rows])


def test_per_point_unit_of_the_oracle(locref, inputs, restated):
    """The oracle's own worst per-point error against the restatement in units of u·κ, over both input sets: the unit of the GPU's
    per-point bar (8 units). The recorded cases.UNIT may not be smaller than what is measured here. Also the conditions of the input."""
    worst = {m: dict(H=0.0, B=0.0) for m in cases.ORACLE_METHODS + (cases.MAPPLANE,)}
    for name, inp in inputs.items():
        for method in cases.ORACLE_METHODS + (cases.MAPPLANE,):
            pp = restated[name, method]
            if method == cases.MAPPLANE:
                table = dict(n4=restated[name, "planes"][0], valid=restated[name, "planes"][1])
                H, B, eff = _one_point_rows(lambda s: map_plane_ref.hb(locref, inp["tree"], table, s, inp["pose"], approximate=inp["approximate"]), inp["scan"])
            else:
                icp = locref.Icp(method=method, use_ann=inp["approximate"])
                icp.set_target(inp["map"])
                H, B, eff = _one_point_rows(lambda s: icp.hb(s, inp["pose"]), inp["scan"])
            ex = cases.excluded(pp)
            keep = ~ex
            # conditions of the input
            if inp["kind"] is None:
                assert ex.mean() <= cases.MAX_EXCLUDED and pp["accepted"].sum() >= cases.MIN_ACCEPTED, (name, method)
            else:
                allowed = np.isin(inp["kind"], [cases.KINDS.index(k) for k in cases.EXACT_KINDS])
                assert not (ex & ~allowed).any(), (name, method)
                assert pp["fitted"][keep].all() and pp["accepted"][keep].all()  # every kind is fitted and accepted
                assert pp["kappa"][keep].max() < cases.KAPPA_MAX
            # the integers are exact away from the gates
            assert np.array_equal(eff[keep], pp["fitted"][keep].astype(int)), (name, method)
            witness = eff > 0 if method == cases.P2P else H.reshape(len(H), -1).any(axis=1)
            assert np.array_equal(witness[keep], pp["accepted"][keep]), (name, method)
            eh, eb = ref.point_errors(H, B, pp)
            uh, ub = cases.units(H, B, pp)
            print("%-9s %-9s fitted %3d accepted %3d excluded %2d  kappa %.3g … %.3g  raw H %.2e B %.2e  in units of u·kappa: H %.3g (median %.2g), B %.3g"
                  % (name, cases.NAMES[method], pp["fitted"].sum(), pp["accepted"].sum(), ex.sum(), pp["kappa"][keep].min(), pp["kappa"][keep].max(),
                     eh[keep].max(), eb[keep].max(), uh[keep].max(), np.median(uh[keep]), ub[keep].max()))
            if inp["kind"] is not None:
                for k, kname in enumerate(cases.KINDS):
                    sel = keep & (inp["kind"] == k)
                    if sel.any():
                        print("    %-16s kappa %.3g … %.3g  raw H %.2e  units H %.3g, B %.3g" % (kname, pp["kappa"][sel].min(), pp["kappa"][sel].max(), eh[sel].max(), uh[sel].max(), ub[sel].max()))
            worst[method]["H"] = max(worst[method]["H"], uh[keep].max())
            worst[method]["B"] = max(worst[method]["B"], ub[keep].max())
    for method, w in worst.items():
        rec = cases.UNIT[method]
        print("per-point unit %-9s: measured H %.4g, B %.4g; recorded H %.3g, B %.3g → GPU bars %.3g, %.3g units of u·kappa"
              % (cases.NAMES[method], w["H"], w["B"], rec["H"], rec["B"], cases.BAR_FACTOR * rec["H"], cases.BAR_FACTOR * rec["B"]))
    for method, w in worst.items():
        # the recorded unit covers the measured one and is no less than 1 (recorded: the measurement rounded up to two digits; another
        # compiler may round the oracle's sums a little differently, which must not fail this test as long as the bar stands on a measurement)
        rec = cases.UNIT[method]
        assert w["H"] <= rec["H"] and w["B"] <= rec["B"] and rec["H"] >= 1 and rec["B"] >= 1, (method, w)


def test_oracle_fits_against_the_exact_vectors(locref, small_world, inputs):
    """locref.fit_plane / fit_line against the exact vectors, in units of u·κ: on the exact 5-NN of 512 map points and of every designed
    map point (what the plane table fits) and on the neighbourhoods of the small-world sample. The units of the table test."""
    worst = dict(n4=0.0, line_d=0.0)
    sets = []
    small, des = inputs["true_pose"], inputs["designed"]
    rows = np.arange(len(small["map"]))[::391][:512]
    sets.append(("table rows, small world", small["map"], cases.exact_neighbourhoods(small["tree"], small["map"], rows)))
    sets.append(("table rows, designed", des["map"], cases.exact_neighbourhoods(des["tree"], des["map"], np.arange(len(des["map"])))))
    sets.append(("sample at true_pose", small["map"], cases.neighbours(locref, small["tree"], small["scan"], small["pose"], cases.P2PLANE)))
    for tag, m, nn in sets:
        m64 = np.asarray(m, dtype=np.float32)[:, :3].astype(np.float64)
        t = ref.plane_table(m, nn)
        keep = ~((t["gates"] <= cases.GATE_REL).any(axis=1) | ~(t["kappa"] <= cases.KAPPA_MAX) | t["rank_deficient"])
        fits = [locref.fit_plane(m64[row]) for row in nn]
        assert np.array_equal(np.array([f[0] for f in fits])[keep], t["valid"][keep])  # validity is exact away from the gate
        un = ref.in_units(ref.vector_errors(np.stack([f[1] for f in fits]), t["n4"], t["n4_lo"]), t["kappa"])
        print("%-24s fit_plane: %d neighbourhoods, %d excluded, valid %d, kappa %.3g … %.3g, |dn4| in units of u·kappa: worst %.3g, median %.2g"
              % (tag, len(nn), (~keep).sum(), t["valid"].sum(), t["kappa"][keep].min(), t["kappa"][keep].max(), un[keep].max(), np.median(un[keep])))
        worst["n4"] = max(worst["n4"], un[keep].max())
        # the line direction of the same neighbourhoods
        pose_free = ref.per_point(ref.P2LINE, m, nn, m64[nn[:, 0]].astype(np.float32), IDENT, max_line_distance=1e30)
        lk = pose_free["kappa"] <= cases.KAPPA_MAX
        d = np.stack([locref.fit_line(m64[row], eps=1e30)[2] for row in nn])
        ul = ref.in_units(ref.vector_errors(d, pose_free["vec"][:, :3], pose_free["vec_lo"][:, :3]), pose_free["kappa"])
        print("%-24s fit_line: kappa_line %.3g … %.3g, |dd| in units of u·kappa_line: worst %.3g, median %.2g"
              % (tag, pose_free["kappa"][lk].min(), pose_free["kappa"][lk].max(), ul[lk].max(), np.median(ul[lk])))
        worst["line_d"] = max(worst["line_d"], ul[lk].max())
    for key, w in worst.items():
        print("unit %s: measured %.3g, recorded %.3g" % (key, w, cases.UNIT[key]))
        assert w <= cases.UNIT[key] and cases.UNIT[key] >= 1
