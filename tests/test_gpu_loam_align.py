"""The LOAM matcher's device-side loop (locgpu_loam_*, csrc/loam_align.hip + loam_solve_kernel) against the oracle composition of
tests/loam_ref.py on the small world's edge / surface split: the joint evaluation, ScanMatch whole, the reference's failure rule, one
class switched off, the batched mode and the error returns."""
import ctypes

import numpy as np
import pytest

import loam_ref
from conftest import pose_delta

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4    # the project's pose bar (tests/test_gpu_parity.py), metres
POSE_TOL_RAD = 1e-4  # ... radians
HB_RTOL = 1e-9       # the project's H/B bar


def _hb_close(Hg, Bg, Ho, Bo):
    """H to 1e-9 of max|H|; B to 1e-9 of the scale the project's H/B tests give it (max|B|, or 1e-6 max|H| where B nearly cancels)."""
    dh, scale = np.abs(Hg - Ho).max(), max(np.abs(Ho).max(), 1e-300)
    db, scale_b = np.abs(Bg - Bo).max(), max(np.abs(Bo).max(), np.abs(Ho).max() * 1e-6, 1e-300)
    print("H/B: max|dH| / max|H| = %.3e, max|dB| / scale = %.3e" % (dh / scale, db / scale_b))
    assert dh <= HB_RTOL * scale and db <= HB_RTOL * scale_b, (dh / scale, db / scale_b)


def _pose_close(got, want, what=""):
    dt, dr = pose_delta(got, want)
    print("pose %s: dt = %.3e m, dr = %.3e rad" % (what, dt, dr))
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (what, dt, dr)


@pytest.fixture(scope="module")
def world(small_world, locref):
    """The split, the oracle with both targets set, and the oracle's run from the initial pose — computed once, never modified."""
    w = loam_ref.split_world(small_world)
    w["oracle"] = loam_ref.LoamOracle(locref, w["edge_map"], w["surf_map"])
    w["run"] = w["oracle"].scan_match(w["edge"], w["surf"], w["init"])
    assert w["run"]["status"] == 0 and w["run"]["iterations"] > 1
    return w


@pytest.fixture(scope="module")
def loam(api, world):
    h = api.Loam()
    h.set_target(world["edge_map"], world["surf_map"])
    yield h
    h.close()


def test_hb_is_the_sum_of_the_two_classes(loam, world):
    o = world["oracle"]
    # the last case leaves the edge class ONE partial block against dozens for the surface class
    for what, edge, pose in (("init", world["edge"], world["init"]), ("converged", world["edge"], world["run"]["pose"]), ("50 edge points", world["edge"][:50], world["init"])):
        H, B, eff, ok = loam.hb(edge, world["surf"], pose)
        Ho, Bo, eff_o, ok_o = o.hb(edge, world["surf"], pose)
        print(what, "eff", eff, "ok", ok)
        assert eff == eff_o and ok == ok_o, (what, eff, eff_o, ok, ok_o)
        _hb_close(H, B, Ho, Bo)


def test_scan_match_equals_the_oracle_composition(loam, world, locref):
    want = world["run"]
    pose, st, cloud = loam.scan_match(world["edge"], world["surf"], world["init"])
    print("iterations", st["iterations"], "oracle", want["iterations"], st)
    _pose_close(pose, want["pose"])
    assert st["status"] == 0 and st["iterations"] == want["iterations"] and st["converged"] == want["converged"]
    both = np.vstack([world["edge"][:, :3], world["surf"][:, :3]])
    np.testing.assert_array_equal(cloud.view(np.uint32), locref.transform_cloud_f32(pose, both).view(np.uint32))
    pose2, st2, cloud2 = loam.scan_match(world["edge"], world["surf"], world["init"])
    assert np.array_equal(pose.view(np.uint64), pose2.view(np.uint64)) and st2 == st
    assert np.array_equal(cloud.view(np.uint32), cloud2.view(np.uint32))


@pytest.mark.parametrize("failing", ["edge", "surf"])
def test_a_false_class_ends_the_alignment_and_leaves_the_outputs(loam, world, failing):
    o = world["oracle"]
    edge, surf = (world["edge"][:5], world["surf"]) if failing == "edge" else (world["edge"], world["surf"][:5])
    assert np.isfinite(edge).all() and np.isfinite(surf).all()
    icp, five = (o.edge_icp, edge) if failing == "edge" else (o.surf_icp, surf)
    assert icp.hb(five, world["init"])[0] is False  # at most 5 effective points < min_effective_pts = 10
    sentinel = np.array([0.5, -0.5, 0.5, -0.5, 11.0, 12.0, 13.0])
    out = np.full((len(edge) + len(surf), 3), 7.5, np.float32)
    pose, st, cloud = loam.scan_match(edge, surf, world["init"], result_pose=sentinel, out_cloud=out)
    assert st["status"] == (4 if failing == "edge" else 3) and st["iterations"] == 1 and not st["converged"], st
    assert np.array_equal(pose, sentinel)
    assert cloud is out and (out == 7.5).all()


@pytest.mark.parametrize("off", ["edge", "surf"])
def test_one_class_switched_off(api, world, off):
    o = world["oracle"]
    edge, surf = (None, world["surf"]) if off == "edge" else (world["edge"], None)
    want = o.scan_match(edge, surf, world["init"])
    h = api.Loam(api.loam_opts(use_edge_points=int(off != "edge"), use_surf_points=int(off != "surf")))
    try:
        h.set_target(None if off == "edge" else world["edge_map"], None if off == "surf" else world["surf_map"])
        pose, st, cloud = h.scan_match(edge, surf, world["init"])
        print(off, "off: iterations", st["iterations"], "oracle", want["iterations"], "status", st["status"], want["status"])
        assert st["status"] == want["status"] == 0 and st["iterations"] == want["iterations"] and st["converged"] == want["converged"]
        _pose_close(pose, want["pose"], off + " off")
        H, B, eff, ok = h.hb(edge, surf, world["init"])
        Ho, Bo, eff_o, ok_o = o.hb(edge, surf, world["init"])
        assert eff == eff_o and ok == ok_o
        _hb_close(H, B, Ho, Bo)
    finally:
        h.close()


def test_batch_every_scan_runs_and_leaves_its_own_loop(loam, world, locref):
    o, init = world["oracle"], world["init"]
    inits = [init, locref.apply_update(init, np.array([0.0, 0.0, 0.004, 0.03, -0.02, 0.0])), locref.apply_update(init, np.array([0.003, -0.002, 0.0, -0.05, 0.04, 0.02])),
             init, init]
    edges = [world["edge"]] * 3 + [world["edge"][:5], world["edge"][:50]]
    surfs = [world["surf"]] * 5
    want = [world["run"]] + [o.scan_match(e, s, p) for e, s, p in list(zip(edges, surfs, inits))[1:]]
    print("oracle: iterations", [w["iterations"] for w in want], "status", [w["status"] for w in want])
    assert want[3]["status"] == 4 and want[3]["iterations"] == 1
    poses, stats = loam.align_batch(edges, surfs, np.array(inits))
    print("gpu:    iterations", [s["iterations"] for s in stats], "status", [s["status"] for s in stats])
    for i, (w, s) in enumerate(zip(want, stats)):
        assert s["status"] == w["status"] and s["iterations"] == w["iterations"] and s["converged"] == w["converged"], (i, s, w)
        _pose_close(poses[i], w["pose"], "scan %d" % i)
    assert np.array_equal(poses[3], inits[3])  # the failed scan hands back its init_pose, bit for bit
    poses2, stats2 = loam.align_batch(edges, surfs, np.array(inits))
    assert np.array_equal(poses.view(np.uint64), poses2.view(np.uint64)) and stats2 == stats


def test_errors_return_the_documented_status(api, world):
    L = api.lib()
    invalid, no_target = -1, -3
    pose = np.array(world["init"])
    out = np.zeros(7)
    e, s = np.ascontiguousarray(world["edge"][:64, :3], np.float32), np.ascontiguousarray(world["surf"][:64, :3], np.float32)
    h = api.Loam()
    try:
        with pytest.raises(api.LocGpuError) as err:
            h.scan_match(e, s, pose)
        assert err.value.code == no_target
        with pytest.raises(api.LocGpuError) as err:
            h.hb(e, s, pose)
        assert err.value.code == no_target
        h.set_target(world["edge_map"][:2000], world["surf_map"][:20000])
        ptrs = (ctypes.c_void_p * 1)(e.ctypes.data)
        ptrs_s = (ctypes.c_void_p * 1)(s.ctypes.data)
        cnts = (ctypes.c_size_t * 1)(64)
        for n in (0, -3):
            assert L.locgpu_loam_align_batch(h._h, n, ptrs, cnts, ptrs_s, cnts, 12, pose.ctypes.data, out.ctypes.data, None) == invalid
        assert L.locgpu_loam_align_batch(h._h, 1, ptrs, cnts, ptrs_s, cnts, 12, None, out.ctypes.data, None) == invalid
        assert L.locgpu_loam_scan_match(h._h, e.ctypes.data, 64, s.ctypes.data, 64, 12, pose.ctypes.data, None, None, None, 0) == invalid
        # an enabled class without its scans is refused, not read
        assert L.locgpu_loam_align_batch(h._h, 1, None, None, ptrs_s, cnts, 12, pose.ctypes.data, out.ctypes.data, None) == invalid
        # the handle is still good
        pose1, st, _ = h.scan_match(e, s, pose)
        assert st["iterations"] >= 1
    finally:
        h.close()
    with pytest.raises(api.LocGpuError) as err:
        api.Loam(api.loam_opts(surf=api.icp_opts(method=api.P2PLANE_MAP)))
    assert err.value.code == invalid
    assert L.locgpu_loam_scan_match(None, e.ctypes.data, 64, s.ctypes.data, 64, 12, pose.ctypes.data, out.ctypes.data, None, None, 0) == invalid
    assert L.locgpu_loam_set_target(None, e.ctypes.data, 64, s.ctypes.data, 64, 12) == invalid
