"""The oracle's one-iteration NDT sums (locref.Ndt.hb) against tests/ndt_hb_ref.py, the long-double restatement the GPU tests of
locgpu_ndt_hb compare per point — closed forms first, then the small world; and the per-point unit of tests/test_gpu_ndt_hb.py."""
import numpy as np
import pytest

import ndt_hb_cases as cases
import ndt_hb_ref as ref
from test_gpu_parity import HB_RTOL, _hb_close

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


@pytest.fixture(scope="module")
def targets(locref, synth, small_world):
    return {name: cases.oracle_target(locref, synth, small_world, name) for name in cases.CASES}


# ---- closed forms of the restatement
def test_identity_pose_one_voxel_direct_and_weighted():
    info = np.array([[2.0, 0.5, 0.0], [0.5, 3.0, 0.25], [0.0, 0.25, 1.0]])
    t = ref.Table([(2, 3, 4)], [(2.5, 3.25, 4.75)], [info])
    p = np.array([[2.25, 3.5, 4.5]], np.float32)
    q = p[0].astype(np.float64)
    e = q - [2.5, 3.25, 4.75]
    hatq = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
    J = np.hstack([-hatq, np.eye(3)])  # every number here is a short dyadic fraction: the products below are exact in FP64
    for weighted, W in ((False, np.eye(3)), (True, info)):
        pp = ref.per_point(t, p, IDENT, n_nearby=1, weighted=weighted)
        assert pp["n_acc"].tolist() == [1] and float(pp["res"][0, 0]) == e @ info @ e
        np.testing.assert_array_equal(pp["H"][0].astype(np.float64), J.T @ W @ J)
        np.testing.assert_array_equal(pp["B"][0].astype(np.float64), -(J.T @ W @ e))


def test_gate_probe_order_truncation_and_points_without_a_voxel():
    t = ref.Table([(0, 0, 0), (1, 0, 0)], [(0.0, 0.0, 0.0), (1.5, 0.5, 0.5)], [np.eye(3), np.eye(3)])
    pts = np.array([[0.5, 0.0, 0.0], [-0.5, -0.5, 0.5], [0.75, 0.5, 0.5], [np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, 0, 0], [3e7, 0, 0], [1e30, 0, 0]], np.float32)
    pp = ref.per_point(t, pts, IDENT, res_outlier_th=0.25)
    # ‖e‖² = 0.25 exactly: `res > th` keeps it; (−1, 1) is one voxel per axis; the third point sees its own voxel (1.0625: gated) and
    # the +x neighbour (0.5625: gated as well)
    assert pp["n_acc"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert float(pp["res"][0, 0]) == 0.25 and float(pp["res"][1, 0]) == 0.75
    assert float(pp["res"][2, 0]) == 1.0625 and float(pp["res"][2, 2]) == 0.5625 and np.isnan(pp["res"][2, 1])
    assert ref.near_gate(pp["res"], 0.25).tolist() == [True] + [False] * 7
    assert np.isnan(pp["res"][3:]).all() and not pp["H"][1:].any() and not pp["B"][1:].any()
    both = ref.per_point(t, pts, IDENT, res_outlier_th=0.6)
    assert both["n_acc"].tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and both["accept"][2].tolist() == [False, False, True, False, False, False, False]
    assert ref.per_point(t, pts, IDENT, res_outlier_th=0.6, n_nearby=1)["n_acc"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_rotation_is_the_oracles(locref):
    pose = np.array([0.02, -0.03, 0.3, 0.0, 1.5, -2.5, 0.25])
    pose[3] = np.sqrt(1 - (pose[:3] ** 2).sum())
    pts = np.array([[1.0, 2.0, 3.0], [-30.5, 12.25, 0.75]])
    want = locref.transform_points(pose, pts)
    got = (pts.astype(ref.LD) @ ref.rotation(pose).T + pose[4:].astype(ref.LD)).astype(np.float64)
    assert np.abs(got - want).max() <= 1e-14


# ---- the small world: the restatement summed over a scan is the oracle's evaluation
@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_summed_equals_oracle_hb(locref, small_world, targets, name):
    ndt, scan, pose = targets[name], small_world["scan10k"], small_world["init_pose"]
    ok, Ho, Bo, eff = ndt.hb(scan, pose)
    pp = cases.restate(ndt, name, scan, pose)
    Hr, Br, pairs = ref.totals(pp)
    Hr, Br = Hr.astype(np.float64), Br.astype(np.float64)
    scale = np.abs(Ho).max()
    print("%s: |H-H_ref|/max|H| = %.2e (bar %.0e), |B-B_ref| = %.2e (|B| %.2e), accepted pairs %d of %d found, effective_num %d"
          % (name, np.abs(Hr - Ho).max() / scale, HB_RTOL, np.abs(Br - Bo).max(), np.abs(Bo).max(), pairs, int((~np.isnan(pp["res"])).sum()), eff))
    _hb_close(Hr, Br, Ho, Bo)
    assert ok
    assert not ref.near_gate(pp["res"], cases.CASES[name][2], cases.GATE_REL).any()  # then the counts below are exact on either side
    assert cases.accepted_pairs(name, Ho, eff) == pairs
    if cases.CASES[name][0] == 1:
        assert eff == len(scan)  # direct: once per source point (ndt cpp:432)
    # the first trace row of an alignment from the same pose is this evaluation, bit for bit (one loop body behind both)
    row = ndt.align(scan, pose, trace_cap=1)["trace"][0]
    assert row[:36].tobytes() == Ho.tobytes() and row[36:42].tobytes() == Bo.tobytes() and row[48] == eff and bool(row[49]) == ok
    if cases.CASES[name][2] == 5.0:  # at the true pose this gate refuses a sizeable share of the residuals, and keeps one
        at_true = cases.restate(ndt, name, scan, small_world["true_pose"])
        share = 1.0 - at_true["n_acc"].sum() / (~np.isnan(at_true["res"])).sum()
        print("%s: share of the found residuals the gate refuses at the true pose %.2f" % (name, share))
        assert 0.2 < share < 0.9


def test_per_point_unit_of_the_oracle(locref, small_world, targets):
    """The oracle's own worst per-point error against the restatement, over the sample of the GPU test and every case: the unit of its
    per-point bar (8 units). The recorded cases.UNIT may not be smaller than what is measured here."""
    pts, pose = cases.sample_points(small_world)
    assert len(pts) == 512
    worst = {1: [0.0, 0.0], 2: [0.0, 0.0]}
    for name in cases.CASES:
        ndt = targets[name]
        pp = cases.restate(ndt, name, pts, pose)
        excluded = ref.near_gate(pp["res"], cases.CASES[name][2], cases.GATE_REL)
        assert excluded.mean() <= cases.MAX_EXCLUDED  # a condition of the input
        rows = [ndt.hb(pts[i:i + 1], pose) for i in range(len(pts))]
        H = np.stack([r[1] for r in rows])
        B = np.stack([r[2] for r in rows])
        got = np.array([cases.accepted_pairs(name, r[1], r[3]) for r in rows])
        assert np.array_equal(got[~excluded], pp["n_acc"][~excluded])
        eh, eb = ref.point_errors(H, B, pp)
        print("%s: oracle per point vs long double: H %.3e, B %.3e; points with an accepted voxel %d / 512, accepted pairs %d, excluded near the gate %d"
              % (name, eh.max(), eb.max(), int((pp["n_acc"] > 0).sum()), int(pp["n_acc"].sum()), int(excluded.sum())))
        assert (pp["n_acc"] > 0).sum() >= 256
        w = worst[cases.CASES[name][0]]
        w[0], w[1] = max(w[0], eh.max()), max(w[1], eb.max())
    for method, (wh, wb) in worst.items():
        uh, ub = cases.UNIT[method]
        print("per-point unit, method %d: H %.3e, B %.3e (recorded %.2e, %.2e) → GPU bars %.2e, %.2e" % (method, wh, wb, uh, ub, cases.BAR_FACTOR * uh, cases.BAR_FACTOR * ub))
        # the recorded unit covers the measured one (recorded: the measurement rounded up to two digits; another compiler may round the
        # oracle's sums a little differently, which must not fail this test as long as the GPU's bar still stands on a measured unit)
        assert wh <= uh and wb <= ub, (method, wh, wb)
