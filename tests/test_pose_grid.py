"""locgpu_pose_grid (include/locgpu.h): the candidate poses of an initial-pose search, a host helper that needs no device and no
context. Checked against a numpy restatement of its definition: centre ∘ (yaw about the centre's z, then x / y offsets in the
centre's frame), yaw-major, then x, then y, each ascending."""
import ctypes

import numpy as np
import pytest


def _quat_mul(a, b):  # Hamilton product, (x, y, z, w)
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _want(centre, xy_half, xy_step, yaw_half, yaw_step):
    kxy = int(np.floor(xy_half / xy_step + 1e-9)) if xy_half > 0 else 0
    kyaw = int(np.floor(yaw_half / yaw_step + 1e-9)) if yaw_half > 0 else 0
    R = _rot(centre[:4])
    out = []
    for a in range(-kyaw, kyaw + 1):
        yaw = a * yaw_step
        q = _quat_mul(centre[:4], np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]))
        for i in range(-kxy, kxy + 1):
            for j in range(-kxy, kxy + 1):
                out.append(np.concatenate([q, centre[4:] + R @ np.array([i * xy_step, j * xy_step, 0.0])]))
    return np.array(out)


def _centre():
    q = np.array([0.02, -0.03, 0.35, 0.93])
    return np.concatenate([q / np.linalg.norm(q), [12.5, -7.25, 1.5]])


def test_pose_grid_matches_its_definition(api):
    c = _centre()
    got, n = api.pose_grid(c, 2.0, 1.0, 0.15, 0.05)
    want = _want(c, 2.0, 1.0, 0.15, 0.05)
    assert n == 175 and got.shape == (175, 7)  # 7 yaws (0.15 / 0.05 divides: ±3 steps) × 5 × 5
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(got[:, :4], axis=1), 1.0, rtol=0, atol=1e-14)
    # ordering: yaw-major, then x, then y — in the centre's frame
    local = (got[:, 4:] - c[4:]) @ _rot(c[:4])
    np.testing.assert_allclose(local[:25, 0], np.repeat([-2.0, -1.0, 0.0, 1.0, 2.0], 5), atol=1e-12)
    np.testing.assert_allclose(local[:25, 1], np.tile([-2.0, -1.0, 0.0, 1.0, 2.0], 5), atol=1e-12)
    np.testing.assert_allclose(local[:, 2], 0.0, atol=1e-12)
    assert all(np.array_equal(got[25 * a, :4], got[25 * a + 24, :4]) for a in range(7))
    assert not np.array_equal(got[0, :4], got[25, :4])
    # the steps divide the halves: the centre is one of the poses, the middle one
    np.testing.assert_allclose(got[87], c, rtol=0, atol=1e-15)


def test_pose_grid_steps_that_do_not_divide_and_single_values(api):
    c = _centre()
    got, n = api.pose_grid(c, 1.7, 0.5, 0.1, 0.04)  # ±3 steps of 0.5 (1.5 <= 1.7), ±2 steps of 0.04
    assert n == 5 * 7 * 7
    np.testing.assert_allclose(got, _want(c, 1.7, 0.5, 0.1, 0.04), rtol=0, atol=1e-12)
    got, n = api.pose_grid(c, 0.0, 0.0, 0.0, 0.0)  # halves of zero: the centre alone, whatever the steps
    assert n == 1
    np.testing.assert_allclose(got[0], c, rtol=0, atol=1e-15)
    got, n = api.pose_grid(c, 0.0, 1.0, 0.2, 0.1)
    assert n == 5 and np.allclose(got[:, 4:], c[4:])


def test_pose_grid_cap_smaller_than_the_count(api):
    c = _centre()
    full, n = api.pose_grid(c, 2.0, 1.0, 0.15, 0.05)
    part, n2 = api.pose_grid(c, 2.0, 1.0, 0.15, 0.05, cap=40)
    assert n2 == n == 175 and part.shape == (40, 7)
    np.testing.assert_array_equal(part, full[:40])
    # a buffer of exactly `cap` poses is never overrun
    buf = np.full((41, 7), -7.0)
    cnt = ctypes.c_size_t(0)
    assert api.lib().locgpu_pose_grid(c.ctypes.data, 2.0, 1.0, 0.15, 0.05, buf.ctypes.data, 40, ctypes.byref(cnt)) == 0
    assert cnt.value == 175 and np.array_equal(buf[:40], full[:40]) and np.all(buf[40] == -7.0)
    # count only
    assert api.lib().locgpu_pose_grid(c.ctypes.data, 2.0, 1.0, 0.15, 0.05, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == 175


@pytest.mark.parametrize("args", [(2.0, 0.0, 0.1, 0.05), (2.0, -1.0, 0.1, 0.05), (-1.0, 1.0, 0.1, 0.05), (2.0, 1.0, 0.1, 0.0),
                                  (float("nan"), 1.0, 0.1, 0.05), (2.0, 1.0, float("inf"), 0.05)])
def test_pose_grid_refuses_bad_steps(api, args):
    with pytest.raises(api.LocGpuError) as e:
        api.pose_grid(_centre(), *args)
    assert e.value.code == -1


def test_init_search_defaults(api):
    o = api.init_search_opts()
    assert (o.max_range, o.min_inlier_ratio) == (1.0, 0.5)
