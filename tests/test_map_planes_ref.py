"""The map-plane mode without a GPU: the CPU restatement (tests/map_plane_ref.py) behaves as its definition says, and the
library's interface carries the three new entry points."""
import os
import re
import subprocess

import numpy as np

import map_plane_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["locgpu_icp_build_map_planes", "locgpu_icp_map_planes_info", "locgpu_icp_map_planes_dump"]


def _plane_cloud(rng, normal, d, n, jitter):
    """n points on the plane normal·p + d = 0 (unit normal) inside a 4 m box, plus jitter along the normal."""
    normal = np.asarray(normal, dtype=np.float64)
    normal /= np.linalg.norm(normal)
    a = np.cross(normal, [0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    b = np.cross(normal, a)
    uv = rng.uniform(-2.0, 2.0, size=(n, 2))
    return uv[:, :1] * a + uv[:, 1:] * b - d * normal + rng.normal(0.0, jitter, size=(n, 1)) * normal


def test_restatement_recovers_analytic_planes(locref):
    rng = np.random.default_rng(11)
    planes = [((0.0, 0.0, 1.0), 0.5, (0.0, 0.0, 0.0)), ((1.0, 0.2, 0.1), -3.0, (40.0, 0.0, 0.0)), ((0.3, -1.0, 0.4), 7.0, (0.0, 60.0, 5.0))]
    clouds, labels = [], []
    for i, (nrm, d, _) in enumerate(planes):
        c = _plane_cloud(rng, nrm, d, 400, 1e-4)  # jitter three orders below the 0.1 m gate
        clouds.append(c)
        labels += [i] * len(c)
    m = np.concatenate(clouds).astype(np.float32)
    labels = np.array(labels)
    tree = locref.KdTree(m)
    t = ref.plane_table(locref, tree, m)
    assert t["leaf"].all() and t["valid"].all()
    np.testing.assert_allclose(np.linalg.norm(t["n4"], axis=1), 1.0, atol=1e-12)  # the 4-vector is unit, the normal is not
    for i, (nrm, d, _) in enumerate(planes):
        nrm = np.asarray(nrm) / np.linalg.norm(nrm)
        truth = np.append(nrm, d) / np.linalg.norm(np.append(nrm, d))  # the analytic plane as a unit 4-vector
        rows = np.flatnonzero(labels == i)
        nb = np.concatenate([m[t["nn"][rows]].astype(np.float64), np.ones((len(rows), 5, 1))], axis=2)
        res_fit = ((nb @ t["n4"][rows][:, :, None])[:, :, 0] ** 2).sum(axis=1)
        res_true = ((nb @ truth) ** 2).sum(axis=1)
        # the fit is the unit 4-vector of least residual over the five neighbours: no worse than the analytic plane, whose residual is
        # the jitter (five points within 5 sigma: at most 5 * (5e-4)^2, scaled by the 4-vector's norm <= 1)
        assert (res_fit <= res_true * (1 + 1e-9) + 1e-18).all()
        assert res_true.max() <= 5 * (5e-4) ** 2
        # ... and it IS that plane up to sign: neighbourhoods are decimetres wide against 0.1 mm of jitter, i.e. a tilt of the order
        # of 1e-3 rad; an order of magnitude of slack on the median (single rows with nearly collinear neighbours may tilt further)
        unit = t["n4"][rows, :3] / np.linalg.norm(t["n4"][rows, :3], axis=1, keepdims=True)
        tilt = np.arccos(np.minimum(1.0, np.abs(unit @ nrm)))
        print("plane %d: median tilt %.2e rad, max %.2e rad" % (i, np.median(tilt), tilt.max()))
        assert np.median(tilt) < 1e-2


def _line(origin, direction, n=50, step=0.5):
    d = np.asarray(direction, dtype=np.float64)
    d /= np.linalg.norm(d)
    return (np.asarray(origin, dtype=np.float64) + step * np.arange(n)[:, None] * d).astype(np.float32), d


def test_restatement_collinear_set_gets_a_degenerate_but_valid_plane(locref):
    """The issue words this case as "a collinear set is invalid". Under the validity rule it states — the reference's own, all five
    (n3·p + d)² <= 1e-2 (math_utils.h:112-136) — that cannot hold: five collinear points make a 5×4 matrix of rank 2, EVERY vector of
    its two-dimensional null space has zero residuals, so whatever null vector the SVD returns passes the rule. The restatement (and
    the library) follow the rule, not the wording: the plane is valid, contains the line, and which of the planes
    through the line it is is not defined. Checked here: validity, zero residuals, a normal perpendicular to the line, d = 0 for a
    line through the origin."""
    line, d = _line((0.0, 0.0, 0.0), (1.0, 0.0, 0.0))  # coordinates exact in float32
    ok, v = locref.fit_plane(line[:5].astype(np.float64))
    assert ok
    t = ref.plane_table(locref, locref.KdTree(line), line)
    assert t["leaf"].all() and t["valid"].all()
    assert t["err2"].max() <= 1e-24             # exact collinear input: residuals at rounding level of the SVD
    assert np.abs(t["n4"][:, :3] @ d).max() <= 1e-12 and np.abs(t["n4"][:, 3]).max() <= 1e-12
    np.testing.assert_allclose(np.linalg.norm(t["n4"], axis=1), 1.0, atol=1e-12)
    # a line in general position: its float32 points lie within sqrt(3)·ulp(4)/2 ≈ 4.2e-7 m of the exact line, so some plane through
    # the exact line has a residual sum <= 5·(4.2e-7)² ≈ 8.7e-13, and the least-squares fit is no worse
    line2, d2 = _line((2.0, 3.0, 1.0), (1.0, 2.0, -1.0), n=9)  # stays inside |coordinate| < 4
    t2 = ref.plane_table(locref, locref.KdTree(line2), line2)
    assert t2["leaf"].all() and t2["valid"].all()
    assert t2["err2"].sum(axis=1).max() <= 1e-12
    # two of the five neighbours are at least 2 steps = 1 m apart along the line and both within sqrt(1e-12) of the plane
    assert np.abs(t2["n4"][:, :3] @ d2).max() <= 2 * 1e-6 / 1.0 + 2 * 4.2e-7


def test_restatement_no_plane_within_the_gate_and_tiny_targets_are_invalid(locref):
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 0.5, 1.5]], np.float32)  # no plane within 0.1 m
    t = ref.plane_table(locref, locref.KdTree(corner), corner)
    assert not t["valid"].any()
    four = corner[:4]
    t = ref.plane_table(locref, locref.KdTree(four), four)
    assert not t["valid"].any() and (t["nn"] == -1).all()
    ok, H, B, eff = ref.hb(locref, locref.KdTree(four), t, corner, np.array([0, 0, 0, 1, 0, 0, 0.0]))
    assert eff == 0 and not ok


def test_restatement_loop_moves_towards_the_true_pose(locref, synth):
    from conftest import pose_delta
    m = synth.make_local_map(60_000, 3, half=25.0)
    s = synth.make_scan(3, subsample=2000, crop_half=22.0)
    true_pose, init_pose = synth.make_pose(3)
    tree = locref.KdTree(m)
    t = ref.plane_table(locref, tree, m)
    assert t["valid"].mean() > 0.5
    r = ref.align(locref, tree, t, s, init_pose)
    d0, d1 = pose_delta(init_pose, true_pose), pose_delta(r["pose"], true_pose)
    print("restatement loop: %d iterations, converged %s, start (%.3f m, %.4f rad) -> end (%.4f m, %.5f rad)" % (r["iters"], r["converged"], *d0, *d1))
    assert d1[0] < d0[0] and d1[1] < d0[1]
    # a NaN source point is no query
    s2 = np.array(s, copy=True)
    s2[3, 1] = np.nan
    assert ref.hb(locref, tree, t, s2, init_pose)[3] <= ref.hb(locref, tree, t, s, init_pose)[3]


def test_new_symbols_are_declared_listed_and_exported(api):
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"LOCGPU_API\s+int\s+%s\s*\(" % name, header), name
        assert name in api.ABI_SYMBOLS
    assert re.search(r"LOCGPU_P2PLANE_MAP\s*=\s*5", header) and api.P2PLANE_MAP == 5
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported
