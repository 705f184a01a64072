"""locgpu_motion_from_poses, the host helper that makes the knots of locgpu_batch_deskew of a pose sequence, against its numpy float64
restatement (tests/motion_ref.py, written line by line from include/locgpu.h): knot times and poses byte for byte. Host code only: the
library is loaded without a device, the way the ABI tests load it."""
import ctypes

import numpy as np
import pytest

import motion_ref as mref

INVALID = -1  # LOCGPU_ERR_INVALID


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(angle / 2.0), [np.cos(angle / 2.0)]])


def _sequence(n, kind, seed):
    """(poses [n, 7], stamps [n]): `rotating` — a random walk of rotations up to 0.3 rad and steps of metres, quaternions unit only to
    rounding and one of them negated; `translation` — one fixed rotation, steps of metres; `constant` — the same twist between every
    pair of consecutive poses."""
    rng = np.random.default_rng(seed)
    stamps = 1.7e9 + np.cumsum(rng.uniform(0.05, 0.15, n))
    poses = np.zeros((n, 7))
    if kind == "constant":
        step = np.concatenate([_quat((0.2, -0.1, 1.0), 0.07), [1.3, -0.4, 0.05]])
        cur = np.concatenate([_quat((1.0, 2.0, 3.0), 0.4), [10.0, -20.0, 1.0]])
        stamps = 100.0 + 0.1 * np.arange(n)
        for i in range(n):
            poses[i] = cur
            cur = mref.compose(step, cur)  # T[i+1] = D * T[i], so T[i+1] * inv(T[i]) = D
        return poses, stamps
    q = _quat(rng.normal(size=3), rng.uniform(0.0, 3.0))
    t = rng.uniform(-50.0, 50.0, 3)
    for i in range(n):
        poses[i, :4], poses[i, 4:] = q, t
        if kind == "rotating":
            q = mref.quat_mul(_quat(rng.normal(size=3), rng.uniform(0.0, 0.3)), q)
        t = t + rng.uniform(-2.0, 2.0, 3)
    if kind == "rotating" and n > 2:
        poses[n // 2, :4] = -poses[n // 2, :4]
    return poses, stamps


@pytest.mark.parametrize("n", [2, 3, 17])
@pytest.mark.parametrize("kind", ["rotating", "translation"])
def test_knots_equal_the_restatement_byte_for_byte(api, n, kind):
    poses, stamps = _sequence(n, kind, 7 * n + len(kind))
    kt, kp = api.motion_from_poses(poses, stamps)
    want_t, want_p = mref.motion_from_poses(poses, stamps)
    assert kt.shape == (n, 3) and kp.shape == (n, 3, 7)
    assert np.array_equal(_bits(kt), _bits(want_t)), (n, kind)
    assert np.array_equal(_bits(kp), _bits(want_p)), (n, kind)
    # the middle knot is the scan's own pose and stamp as given, its neighbours' the neighbours'
    assert np.array_equal(_bits(kp[:, 1]), _bits(poses)) and np.array_equal(_bits(kt[:, 1]), _bits(stamps))
    assert np.array_equal(_bits(kp[1:, 0]), _bits(poses[:-1])) and np.array_equal(_bits(kp[:-1, 2]), _bits(poses[1:]))
    assert (np.diff(kt, axis=1) > 0).all()  # what locgpu_batch_deskew asks of knot times


def test_end_knots_are_the_reference_expression_on_a_constant_velocity_sequence(api):
    poses, stamps = _sequence(6, "constant", 0)
    kt, kp = api.motion_from_poses(poses, stamps)
    after = mref.compose(mref.compose(poses[-1], mref.inverse(poses[-2])), poses[-1])  # result_pos * last_pose.inverse() * result_pos
    before = mref.compose(mref.compose(poses[0], mref.inverse(poses[1])), poses[0])
    assert np.array_equal(_bits(kp[-1, 2]), _bits(after)) and np.array_equal(_bits(kp[0, 0]), _bits(before))
    assert kt[-1, 2] == 2.0 * stamps[-1] - stamps[-2] and kt[0, 0] == 2.0 * stamps[0] - stamps[1]
    # constant velocity: the extrapolated pose continues the sequence — one more step of the same twist, to rounding
    step = mref.compose(poses[1], mref.inverse(poses[0]))
    assert np.abs(after - mref.compose(step, poses[-1])).max() < 1e-12 * 30.0
    assert np.abs(mref.compose(step, before) - poses[0]).max() < 1e-12 * 30.0
    assert np.abs(after[4:] - poses[-1, 4:]).max() > 0.1  # and it does move


def test_refusals(api):
    L = api.lib()
    poses, stamps = _sequence(4, "rotating", 3)
    kt, kp = np.full((4, 3), 7.0), np.full((4, 3, 7), 7.0)

    def text(rc):
        assert rc == INVALID
        t = L.locgpu_last_error(None)
        assert b"motion_from_poses: " in t and len(t) > 20
        return t

    def call(p, s, n, t=kt, q=kp):
        return L.locgpu_motion_from_poses(p.ctypes.data if p is not None else None, s.ctypes.data if s is not None else None, n, t.ctypes.data if t is not None else None,
                                          q.ctypes.data if q is not None else None)

    for n in (1, 0, -3):
        assert b"n < 2" in text(call(poses, stamps, n))
    assert b"NULL" in text(call(None, stamps, 4))
    assert b"NULL" in text(call(poses, None, 4))
    assert b"NULL" in text(call(poses, stamps, 4, t=None))
    assert b"NULL" in text(call(poses, stamps, 4, q=None))
    for i, bad in ((2, np.nan), (3, np.inf), (1, stamps[0]), (3, stamps[1])):
        s = stamps.copy()
        s[i] = bad
        assert b"increasing" in text(call(poses, s, 4))
        with pytest.raises(api.LocGpuError) as err:
            api.motion_from_poses(poses, s)
        assert err.value.code == INVALID and "increasing" in str(err.value)
    with pytest.raises(api.LocGpuError):
        api.motion_from_poses(poses[:1], stamps[:1])
    assert (kt == 7.0).all() and (kp == 7.0).all()  # a refused call writes nothing
    assert call(poses, stamps, 4) == 0 and not (kt == 7.0).any()
