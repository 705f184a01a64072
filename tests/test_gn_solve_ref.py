"""The restatement of the solve stage (tests/gn_solve_ref.py) against the oracle's pieces, what the case sets cover, and the host twin
locgpu_gn_update over the same sets. No GPU.

A. The restated LU equals locref.lu6 bit for bit — x and det — on every matrix of the sets; the restated float64 update equals
   locref.apply_update bit for bit on every update case. From then on the restatement's by-products (pivot rows, zero-pivot steps, which
   branch an update took) describe the oracle's run too.
B. Coverage, from the restatement alone: the pivot set takes all 21 (step, pivot row) choices and has positive semi-definite and indefinite
   members; a zero pivot occurs at every step 0 … 5, by a structural zero and by cancellation; det can underflow to zero with no zero
   pivot; the update cases take the Taylor branch exactly up to the last double below 1e-10 and both sides of `sq != 1.0`; every boundary
   the GPU module sits on (effective count, eps, iteration limit) has a case on either side.
C. locgpu_gn_update over the sets: dx bits = locref.lu6 (÷16 for P2P), pose bits = locref.apply_update, applied / stop by the rules,
   nothing applied and nothing touched for a singular H or too few points, strict `<` at eps = 2^-7, and |dx| summed in the
   association of the device and of the reference's binary: two dx found by search, on which the plain running sum lands one ulp below /
   above it, decide `stop` the way the oracle's norm6 does.
D. The float64 update against the long-double one over the sin/cos cases: the figure the GPU module's bar is built on."""
import math

import numpy as np
import pytest

import gn_solve_cases as cases
import gn_solve_ref as ref

ICP_METHODS = (ref.P2P, ref.P2LINE, ref.P2PLANE, ref.P2PLANE_MAP)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def all_matrices():
    return cases.pivot_cases() + cases.singular_cases() + (cases.regular_case(0), cases.regular_case(1))


# ----------------------------------------------------------------------------------------------------------------------------- A
def test_restated_lu_equals_the_oracle_bit_for_bit(locref):
    for c in all_matrices():
        lu = ref.lu6(c.H.tolist(), c.B.tolist())
        det, x = locref.lu6(c.H, c.B)
        assert bits([lu.det])[0] == bits([det])[0], c.name
        assert np.array_equal(bits(lu.x), bits(x)), c.name


def test_restated_update_equals_the_oracle_bit_for_bit(locref):
    for name, q, t, dx in cases.update_cases():
        u = ref.apply_update_f64(q, t, dx)
        want = locref.apply_update(np.array(q + t), np.array(dx))
        assert np.array_equal(bits(u.q + u.t), bits(want)), name


# ----------------------------------------------------------------------------------------------------------------------------- B
def test_pivot_set_takes_every_step_and_row_choice():
    seen, kinds = set(), set()
    for c in cases.pivot_cases():
        lu = ref.lu6(c.H.tolist(), c.B.tolist())
        assert np.array_equal(c.H, c.H.T) and lu.det != 0.0 and not lu.zero_steps, c.name
        ev = np.linalg.eigvalsh(c.H)
        assert (ev.min() > -1e-9 * ev.max()) == (c.kind == "psd"), c.name
        seen |= set(enumerate(lu.pivots))
        kinds.add(c.kind)
    assert seen == cases.ALL_PIVOT_PAIRS and len(seen) == 21
    assert kinds == {"psd", "indefinite"}
    assert len(cases.pivot_cases()) <= 24


def test_singular_set_has_a_zero_pivot_at_every_step():
    by_name = {c.name: ref.lu6(c.H.tolist(), c.B.tolist()) for c in cases.singular_cases()}
    for name, lu in by_name.items():
        assert lu.det == 0.0 and lu.x == [0.0] * 6, name
    for k in range(6):
        assert by_name["structural%d" % k].zero_steps[0] == k
    for k in range(1, 6):
        assert by_name["cancel%d" % k].zero_steps == [k]
    assert by_name["two_zeros"].zero_steps[:2] == [0, 2]
    assert by_name["underflow"].zero_steps == []  # nothing singular: the product of six pivots of 1e-60 underflows
    # after a zero pivot that is not the last step the factorisation goes on with real numbers: a pivot search, and a swap somewhere
    assert any(lu.zero_steps and lu.zero_steps[0] < 5 and any(p != k for k, p in enumerate(lu.pivots) if k > lu.zero_steps[0]) for lu in by_name.values())


def test_update_set_sits_on_both_sides_of_its_branches():
    by_name = {name: ref.apply_update_f64(q, t, dx) for name, q, t, dx in cases.update_cases()}
    assert len(by_name) == 56
    for name, u in by_name.items():
        tn = name.split("_")[-2]
        assert u.taylor == (tn in ("0", "below")), name
    assert by_name["identity_below_x"].theta == math.nextafter(1e-10, 0.0) and by_name["identity_at_x"].theta == 1e-10
    assert {u.renormalised for u in by_name.values()} == {True, False}
    assert not by_name["identity_0_x"].renormalised and by_name["off_unit_1_mixed"].renormalised
    assert {u.renormalised for n, u in by_name.items() if not u.taylor} == {True, False}


def test_boundaries_have_a_case_on_either_side():
    st0 = ref.make_state()
    for method in ref.METHODS:
        b = 0.125 if method == ref.P2P else 2.0 ** -7  # P2P divides by 16
        tot = cases.identity_row([0, 0, 0, 0, b, 0])[:28]
        at, _, _ = ref.gn_step(tot, st0, method, 10, 2.0 ** -7, 20)
        above, _, _ = ref.gn_step(tot, st0, method, 10, math.nextafter(2.0 ** -7, 1.0), 20)
        assert at["last_dx_norm"] == 2.0 ** -7 and not at["converged"] and not at["done"] and above["converged"] and above["done"], method
        # effective count: min and min − 1
        enough, _, _ = ref.gn_step(cases.identity_row([0, 0, 0, 0, b, 0], eff=10)[:28], st0, method, 10, 1e-9, 20)
        short, _, _ = ref.gn_step(cases.identity_row([0, 0, 0, 0, b, 0], eff=9)[:28], st0, method, 10, 1e-9, 20)
        assert enough["t"][1] == 2.0 ** -7 and short["t"][1] == 0.0 and short["status"] == (2 if method == ref.NDT_INC else 0), method
        # iteration limit
        last, _, _ = ref.gn_step(tot, ref.make_state(iterations=19), method, 10, 1e-9, 20)
        before, _, _ = ref.gn_step(tot, ref.make_state(iterations=18), method, 10, 1e-9, 20)
        assert last["done"] and not last["converged"] and not before["done"], method


def test_reduction_order_differs_from_the_plain_sum_and_stays_within_the_derived_bound():
    """The restated order is not the row-by-row sum (so a test on its bits can tell them apart), and both lie within
    rows · 2^-53 · Σ|row| of the long-double sum."""
    rng = np.random.RandomState(5)
    differs = False
    for blocks in (1, 7, 8, 9, 255, 256, 257, 513):
        rows = cases.spread_rows(rng, 1, blocks)[0]
        got = ref.reduce_f64(rows)
        want, mag = ref.reduce_ld(rows)
        assert (np.abs(got.astype(ref.LD) - want) <= blocks * ref.LD(2.0 ** -53) * mag).all(), blocks
        plain = np.zeros(28)
        for r in rows:
            plain = plain + r[:28]
        differs |= not np.array_equal(bits(plain), bits(got))
        if blocks == 1:
            assert np.array_equal(bits(got), bits(0.0 + rows[0, :28]))
    assert differs


# ----------------------------------------------------------------------------------------------------------------------------- C
def _hb(H, B, eff):
    return np.concatenate([np.asarray(H, dtype=np.float64).reshape(-1), np.asarray(B, dtype=np.float64), [float(eff), 1.0]])


POSES = (np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), np.array([0.5, -0.5, 0.5, 0.5, 1.0, -2.0, 3.0]))


@pytest.mark.parametrize("method", ICP_METHODS)
def test_host_update_over_the_case_set(api, locref, method):
    g = np.array([0.1, -0.2, 0.3, 0.9])
    poses = POSES + (np.concatenate([g / np.linalg.norm(g), [1.0, 2.0, 3.0]]),)
    for c in all_matrices():
        for eff in (10, 9):
            for pose in poses:
                got_pose, got_dx, applied, stop = api.gn_update(_hb(c.H, c.B, eff), method, 10, 1e-2, pose)
                det, x = locref.lu6(c.H, c.B)
                want_pose, want_dx, want_applied, want_stop = ref.host_gn_update(_hb(c.H, c.B, eff), method, 10, 1e-2, pose)
                assert applied == want_applied == (eff >= 10 and det != 0.0), (c.name, eff)
                assert stop == want_stop, (c.name, eff)
                if not applied:
                    assert np.array_equal(bits(got_pose), bits(pose)) and np.array_equal(bits(got_dx), bits(np.zeros(6))), (c.name, eff)
                    continue
                x = x / 16 if method == ref.P2P else x
                assert np.array_equal(bits(got_dx), bits(x)) and np.array_equal(bits(got_dx), bits(want_dx)), (c.name, eff)
                assert np.array_equal(bits(got_pose), bits(locref.apply_update(pose, x))), (c.name, eff)
                assert np.array_equal(bits(got_pose), bits(want_pose)), (c.name, eff)


def test_host_update_on_the_update_cases(api, locref):
    """Every angle and q_in of the update set through the host twin: pose bits = the oracle's (same C library for sin and cos)."""
    for name, q, t, dx in cases.update_cases():
        pose = np.array(q + t)
        got_pose, got_dx, applied, stop = api.gn_update(_hb(np.eye(6), dx, 100), ref.P2PLANE, 10, 1e-2, pose)
        assert applied and np.array_equal(bits(got_dx), bits(dx)), name
        assert np.array_equal(bits(got_pose), bits(locref.apply_update(pose, np.array(dx)))), name


def test_host_update_stops_strictly_below_eps(api):
    for method in ICP_METHODS:
        b = 0.125 if method == ref.P2P else 2.0 ** -7
        hb = _hb(np.eye(6), [0, 0, 0, 0, b, 0], 50)
        _, dx, applied, stop = api.gn_update(hb, method, 10, 2.0 ** -7, POSES[0])
        assert applied and dx[4] == 2.0 ** -7 and not stop, method
        _, _, applied, stop = api.gn_update(hb, method, 10, math.nextafter(2.0 ** -7, 1.0), POSES[0])
        assert applied and stop, method


@pytest.mark.parametrize("running_sum_smaller", [True, False])
def test_host_update_sums_the_norm_as_the_device_and_the_oracle_do(api, running_sum_smaller):
    """|dx| is (d0² + (d2² + d4²)) + (d1² + (d3² + d5²)) in the reference's binary, in the oracle (locref::norm6) and in gn_solve_kernel.
    On these two dx the running sum d0² + d1² + … lands on the neighbouring double, and a `stop` on the boundary would differ: with
    eps = the binary's |dx| the update must not stop (the running sum, where smaller, would); with eps = the running sum's larger value it
    must (the running sum itself would not)."""
    dx, binary, running = cases.norm_split_dx(running_sum_smaller)
    assert binary != running and (running < binary) == running_sum_smaller
    assert abs(binary - running) <= 2 * math.ulp(binary)
    eps = binary if running_sum_smaller else running
    _, got_dx, applied, stop = api.gn_update(_hb(np.eye(6), dx, 50), ref.P2PLANE, 10, eps, POSES[0])
    assert applied and np.array_equal(bits(got_dx), bits(dx))
    assert stop == (binary < eps) == (not running_sum_smaller)
    assert (running < eps) != stop  # the sum this test is about decides the other way


# ----------------------------------------------------------------------------------------------------------------------------- D
def test_float64_update_against_long_double(api):
    """The host twin (CPU libm) against the long-double update over the sin/cos cases: a few 2^-53 at the most — the GPU module adds
    8 · 2^-53 to this figure for the device's sin and cos and keeps the sum at or below 1e-15."""
    restated = cases.trig_update_error(lambda q, t, dx: ref.apply_update_f64(q, t, dx).q)
    host = cases.trig_update_error(lambda q, t, dx: api.gn_update(_hb(np.eye(6), dx, 100), ref.P2PLANE, 10, 1e-2, np.array(q + t))[0][:4])
    print("float64 update against long double over the sin/cos cases: restated %.3e, locgpu_gn_update %.3e (2^-53 = %.3e)" % (restated, host, 2.0 ** -53))
    assert host == restated  # the same expressions and the same C library
    assert host <= 4 * 2.0 ** -53
    # the Taylor cases: nothing but + − × — the long-double result is the float64 one to a rounding or two of each component
    for name, q, t, dx in cases.update_cases():
        u = ref.apply_update_f64(q, t, dx)
        if u.taylor:
            q_ld, t_ld = ref.apply_update_ld(q, t, dx)
            assert float(np.abs(np.array(u.q).astype(ref.LD) - q_ld).max()) <= 4 * 2.0 ** -53, name
            assert float(np.abs(np.array(u.t).astype(ref.LD) - t_ld).max()) <= 2.0 ** -53 * 64, name
