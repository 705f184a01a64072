"""The device Gauss–Newton solve stage — gn_solve_kernel, sum_partials_kernel and loam_solve_kernel (csrc/icp_fit.hip), through their
production launchers (locgpu_debug_gn_solve / locgpu_debug_loam_solve) — on chosen normal equations, against the plain restatement in
tests/gn_solve_ref.py (which tests/test_gn_solve_ref.py holds to the oracle bit for bit, and whose case sets it shows to cover all 21
pivot choices, a zero pivot at every step and both sides of every branch).

What is compared, per scan (check_scan):
    iterations, converged, done, status, last_eff       equal
    t                                                    bits (one addition per component)
    hb row                                               bits (the sum of the block partials in the documented order)
    q after a Taylor-branch update                       bits (+ − × ÷ and sqrt only)
    q after a sin/cos update                             |q − q_ld| ≤ bar against the long-double update, bar = host + 8 · 2^-53 capped
                                                         at the project's 1e-15, host = the same error of locgpu_gn_update (CPU libm)
    R                                                    bits of quat_to_R restated on the q that came back
    last_dx_norm                                         within 1 ulp of the restatement (the distance is printed)
    a scan that is not solved, or solved without update  the bytes that went in

Measured on an MI355X (printed by test_update_cases and its neighbours, -s):
    sin/cos cases against long double   host (locgpu_gn_update, glibc) 2.173e-16, device 2.173e-16: all 40 device q equal the CPU
                                        restatement bit for bit; bar = min(2.173e-16 + 8 · 2^-53, 1e-15) = 1e-15
    last_dx_norm                        0 ulp from the restatement over every update of the module (device sqrt and ÷ round correctly
                                        on all of them)
    every bit claim above held          lu6_det_solve_reg on all 21 pivot choices and every zero pivot, the reduction order, R

Every launch has at most 64 scans and at most 513 rows."""
import math

import numpy as np
import pytest

import gn_solve_cases as cases
import gn_solve_ref as ref

pytestmark = pytest.mark.gpu

EPS_NEVER = 0.0  # |dx| < 0 never holds: a scan stays open
INTS = ("iterations", "converged", "done", "status", "last_eff")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulp_distance(a, b):
    """Doubles between two finite non-negative doubles."""
    return abs(int(bits([a])[0]) - int(bits([b])[0]))


def pack_states(api, states):
    out = np.zeros(len(states), dtype=api.SOLVE_STATE)
    for i, s in enumerate(states):
        for k, v in s.items():
            out[i][k] = v
    return out


@pytest.fixture(scope="module")
def bar(api):
    """(bar, host): the device bar of the sin/cos updates and the host figure it is built on."""
    host = cases.trig_update_error(lambda q, t, dx: api.gn_update(np.concatenate([np.eye(6).reshape(-1), dx, [100.0, 1.0]]), ref.P2PLANE, 10, 1e-2, np.array(q + t))[0][:4])
    return min(host + 8 * 2.0 ** -53, 1e-15), host


class Tally:
    def __init__(self):
        self.norm_ulp = 0      # worst distance of last_dx_norm from the restatement
        self.norms = 0         # updates compared
        self.trig_err = 0.0    # worst |q − q_ld| of a sin/cos update
        self.trigs = 0


def check_scan(tag, st_in, got, got_hb, hb_in, want, want_hb, step, bar, tally):
    """One scan of one launch: `got` / `got_hb` from the device, `want` / `want_hb` / `step` from gn_step or loam_step on st_in."""
    if want_hb is None:  # finished before the launch, or not listed: nothing is written
        assert got.tobytes() == st_in.tobytes(), tag
        assert got_hb.tobytes() == hb_in.tobytes(), tag
        return
    assert np.array_equal(bits(got_hb), bits(want_hb)), (tag, got_hb, want_hb)
    for k in INTS:
        assert int(got[k]) == want[k], (tag, k, int(got[k]), want[k])
    assert np.isfinite(got["q"]).all() and np.isfinite(got["t"]).all() and np.isfinite(got["R"]).all() and math.isfinite(got["last_dx_norm"]), tag
    if step is None or step.dx is None:  # no update: pose, R and last_dx_norm as they went in
        for k in ("q", "t", "R", "last_dx_norm"):
            assert got[k].tobytes() == st_in[k].tobytes(), (tag, k)
        return
    assert np.array_equal(bits(got["t"]), bits(want["t"])), (tag, got["t"], want["t"])
    if step.update.taylor:
        assert np.array_equal(bits(got["q"]), bits(want["q"])), (tag, got["q"], want["q"])
    else:
        q_ld, _ = ref.apply_update_ld(st_in["q"], st_in["t"], step.dx)
        err = float(np.abs(got["q"].astype(ref.LD) - q_ld).max())
        tally.trig_err = max(tally.trig_err, err)
        tally.trigs += 1
        assert err <= bar[0], (tag, err, bar)
    assert np.array_equal(bits(got["R"]), bits(ref.quat_to_R(got["q"]))), tag
    d = ulp_distance(float(got["last_dx_norm"]), want["last_dx_norm"])
    tally.norm_ulp = max(tally.norm_ulp, d)
    tally.norms += 1
    assert d <= 1, (tag, float(got["last_dx_norm"]), want["last_dx_norm"])


def run_gn(api, ctx, partials, states, method, bar, tally, min_eff=10, eps=EPS_NEVER, max_it=20, do_update=True, two_stage=False, scans=None, tag=""):
    """One launch of the solve on `partials` [n, blocks, 32] and every scan compared with gn_step. → (state_out, hb_out, wanted states)"""
    st_in = pack_states(api, states)
    hb_in = np.full((len(states), ref.HB_W), -7.25)
    got, hb = ctx.debug_gn_solve(partials, st_in, method, min_effective_pts=min_eff, eps=eps, max_iteration=max_it, do_update=do_update, two_stage=two_stage,
                                 scans=scans, hb=hb_in)
    wants = []
    for i, s in enumerate(states):
        if scans is not None and i not in scans:
            want, want_hb, step = s, None, None
        else:
            want, want_hb, step = ref.gn_step(ref.reduce_f64(partials[i]), s, method, min_eff, eps, max_it, do_update)
        check_scan("%s scan %d method %d" % (tag, i, method), st_in[i], got[i], hb[i], hb_in[i], want, want_hb, step, bar, tally)
        wants.append(want)
    return got, hb, wants


def one_row(cs, eff=100):
    return np.stack([ref.pack_row(c.H, c.B, eff) for c in cs])[:, None, :]


# ------------------------------------------------------------------------------------------------------------------------- LU
@pytest.mark.parametrize("method", ref.METHODS)
def test_lu_bits_on_the_pivot_set(api, gpu_ctx, locref, bar, method):
    """All 21 (step, pivot row) choices of lu6_det_solve_reg: with q = identity and t = 0 going in, t coming out IS x[3:6] — bit for bit
    the oracle's (÷16 for P2P)."""
    cs = cases.pivot_cases() + (cases.regular_case(0), cases.regular_case(1))
    tally = Tally()
    got, hb, _ = run_gn(api, gpu_ctx, one_row(cs), [ref.make_state() for _ in cs], method, bar, tally, tag="pivot")
    for i, c in enumerate(cs):
        det, x = locref.lu6(c.H, c.B)
        assert det != 0.0
        x = x / 16 if method == ref.P2P else x
        assert np.array_equal(bits(got[i]["t"]), bits(0.0 + x[3:6])), (c.name, got[i]["t"], x[3:6])
        assert got[i]["iterations"] == 1 and not got[i]["done"] and hb[i][43] == 1.0
    assert tally.norms == len(cs)
    print("pivot set, method %d: last_dx_norm at most %d ulp from the restatement; sin/cos q error %.3e (bar %.3e)" % (method, tally.norm_ulp, tally.trig_err, bar[0]))


# -------------------------------------------------------------------------------------------------------- singular H, zero pivots
@pytest.mark.parametrize("method", ref.METHODS)
def test_singular_h_and_zero_pivots(api, gpu_ctx, bar, method):
    """det(H) == 0 with the zero pivot at every step 0 … 5 (0/0 in the elimination unless the `nz` selects hold it back), twice, and by
    underflow alone. ICP: an iteration without an update. Direct NDT: status 1, done. Incremental NDT: no test of det — the oracle's rule
    updates with dx = 0 and stops on |dx| = 0 < eps. Exactly unit q going in: the pose comes back byte for byte."""
    cs = cases.singular_cases()
    q = cases.UNIT_QS[1][1]
    states = [ref.make_state(q=q if i % 2 else cases.UNIT_QS[0][1], t=(1.0, -2.0, 3.5), last_dx_norm=0.5, iterations=3) for i in range(len(cs))]
    tally = Tally()
    got, hb, _ = run_gn(api, gpu_ctx, one_row(cs), states, method, bar, tally, eps=1e-2, tag="singular")
    st_in = pack_states(api, states)
    for i, c in enumerate(cs):
        assert got[i]["q"].tobytes() == st_in[i]["q"].tobytes() and got[i]["t"].tobytes() == st_in[i]["t"].tobytes(), c.name
        assert got[i]["R"].tobytes() == st_in[i]["R"].tobytes() and got[i]["iterations"] == 4 and got[i]["last_eff"] == 100, c.name
        if method == ref.NDT_DIRECT:
            assert (got[i]["status"], got[i]["done"], got[i]["converged"], hb[i][43]) == (1, 1, 0, 0.0), c.name
        elif method == ref.NDT_INC:
            assert (got[i]["status"], got[i]["done"], got[i]["converged"], hb[i][43], got[i]["last_dx_norm"]) == (0, 1, 1, 1.0, 0.0), c.name
        else:
            assert (got[i]["status"], got[i]["done"], got[i]["converged"], hb[i][43], got[i]["last_dx_norm"]) == (0, 0, 0, 0.0, 0.5), c.name


# ----------------------------------------------------------------------------------------------------------------- boundaries
@pytest.mark.parametrize("method", ref.METHODS)
def test_boundaries(api, gpu_ctx, bar, method):
    """effective_num = min and min − 1; |dx| = 2^-7 exactly against eps = 2^-7 (strict: open) and the next double (converged);
    iterations_in = max_iteration − 1 and − 2. Powers of two keep the square, the sum and the root exact."""
    b = 0.125 if method == ref.P2P else 2.0 ** -7
    row = lambda eff: cases.identity_row([0, 0, 0, 0, b, 0], eff)
    partials = np.stack([row(10), row(9), row(50), row(50), row(50)])[:, None, :]
    states = [ref.make_state(), ref.make_state(), ref.make_state(iterations=19), ref.make_state(iterations=18), ref.make_state(iterations=25)]
    tally = Tally()
    for eps, open_after in ((2.0 ** -7, True), (math.nextafter(2.0 ** -7, 1.0), False)):
        got, hb, _ = run_gn(api, gpu_ctx, partials, states, method, bar, tally, eps=eps, tag="boundary eps %r" % eps)
        assert got[0]["last_dx_norm"] == 2.0 ** -7 and got[0]["t"][1] == 2.0 ** -7
        assert (got[0]["converged"], got[0]["done"]) == ((0, 0) if open_after else (1, 1))
        assert got[1]["t"][1] == 0.0 and got[1]["converged"] == 0 and hb[1][43] == 0.0 and hb[1][42] == 9.0
        assert (got[1]["status"], got[1]["done"]) == ((2, 1) if method == ref.NDT_INC else (0, 0))
        assert got[2]["iterations"] == 20 and got[2]["done"] == 1 and got[2]["converged"] == (0 if open_after else 1)
        assert got[3]["iterations"] == 19 and got[3]["done"] == (0 if open_after else 1)
        assert got[4]["iterations"] == 26 and got[4]["done"] == 1
    assert tally.norm_ulp == 0  # exact operands: any correctly rounded sqrt gives 2^-7


@pytest.mark.parametrize("method", ref.METHODS)
def test_evaluation_without_update_writes_hb_and_last_eff_only(api, gpu_ctx, bar, method):
    cs = (cases.regular_case(0), cases.pivot_cases()[0], cases.regular_case(1))
    partials = one_row(cs)
    partials[2, 0, 27] = 9.0  # too few: ok = 0 for the ICP methods and direct NDT; the incremental variant ends the alignment whatever do_update says
    states = [ref.make_state(q=cases.UNIT_QS[1][1], t=(1.0, 2.0, 3.0), last_dx_norm=0.25, last_eff=77, iterations=5) for _ in cs]
    tally = Tally()
    got, hb, _ = run_gn(api, gpu_ctx, partials, states, method, bar, tally, do_update=False, eps=1e9, max_it=1, tag="no update")
    st_in = pack_states(api, states)
    for i in range(3):
        if i == 2 and method == ref.NDT_INC:
            continue
        want = st_in[i].copy()
        want["last_eff"] = 9 if i == 2 else 100
        assert got[i].tobytes() == want.tobytes(), i
        assert hb[i][43] == (0.0 if i == 2 else 1.0) and np.array_equal(bits(hb[i][:36]), bits(cs[i].H.reshape(-1)))
    assert tally.norms == 0


# ------------------------------------------------------------------------------------------------------------------------ update
def test_update_cases(api, gpu_ctx, bar):
    """theta = 0, the last double below 1e-10, 1e-10, 1e-3, 1, π, 2π − 1e-6, about x and about a general axis, on q = identity, an exactly
    unit q, a normalised q and one off-unit by 1e-12 (56 scans, one launch; H = I, so dx is the right-hand side itself)."""
    ucs = cases.update_cases()
    partials = np.stack([cases.identity_row(dx) for _, _, _, dx in ucs])[:, None, :]
    states = [ref.make_state(q=q, t=t) for _, q, t, _ in ucs]
    tally = Tally()
    got, hb, wants = run_gn(api, gpu_ctx, partials, states, ref.P2PLANE, bar, tally, tag="update")
    taylor = [ref.apply_update_f64(q, t, dx).taylor for _, q, t, dx in ucs]
    for i, (name, q, t, dx) in enumerate(ucs):
        if taylor[i]:
            assert np.array_equal(bits(got[i]["q"]), bits(wants[i]["q"])), name
    same = sum(np.array_equal(bits(got[i]["q"]), bits(wants[i]["q"])) for i in range(len(ucs)) if not taylor[i])
    print("sin/cos update cases: host (locgpu_gn_update, CPU libm) %.3e, device %.3e against long double; bar %.3e = min(host + 8 * 2^-53, 1e-15); "
          "%d of %d device q equal the CPU restatement bit for bit" % (bar[1], tally.trig_err, bar[0], same, tally.trigs))
    print("last_dx_norm: at most %d ulp from the float64 restatement over %d updates" % (tally.norm_ulp, tally.norms))
    assert tally.trigs == sum(not t for t in taylor) == 40 and tally.norms == 56
    assert bar[0] <= 1e-15 and tally.trig_err <= bar[0]


# --------------------------------------------------------------------------------------------------------------------- reduction
@pytest.mark.parametrize("blocks", [1, 7, 8, 9, 255, 256, 257, 513])
def test_reduction_order(api, gpu_ctx, bar, blocks):
    """Row counts around the 8 chunks and the 256 rows of a round: hb's H and B are the restated order's sums bit for bit (NaN in the
    spare columns stays out), each within rows · 2^-53 · Σ|row| of the long-double sum, and the sharded route — sum_partials_kernel into
    one row per scan, then the solve on that row — gives the same bytes, states included."""
    rng = np.random.RandomState(100 + blocks)
    partials = cases.spread_rows(rng, 3, blocks)
    states = [ref.make_state(q=cases.UNIT_QS[i % 2][1], t=(0.5, 0.25, -1.0)) for i in range(3)]
    tally = Tally()
    got, hb, _ = run_gn(api, gpu_ctx, partials, states, ref.P2PLANE, bar, tally, tag="reduce %d" % blocks)
    for i in range(3):
        tot = ref.reduce_f64(partials[i])
        H, B, eff = ref.unpack(tot)
        assert np.array_equal(bits(hb[i][:36]), bits(np.array(H).reshape(-1))) and np.array_equal(bits(hb[i][36:42]), bits(B)) and hb[i][42] == eff
        want, mag = ref.reduce_ld(partials[i])
        dev = np.array([hb[i][6 * r + c] for r in range(6) for c in range(r, 6)] + list(hb[i][36:43]))
        assert (np.abs(dev.astype(ref.LD) - want) <= blocks * ref.LD(2.0 ** -53) * mag).all()
    got2, hb2, _ = run_gn(api, gpu_ctx, partials, states, ref.P2PLANE, bar, tally, two_stage=True, tag="reduce two-stage %d" % blocks)
    assert got2.tobytes() == got.tobytes() and hb2.tobytes() == hb.tobytes()


# ------------------------------------------------------------------------------------------------------------------ mixed launch
def test_finished_and_unlisted_scans_come_back_byte_for_byte(api, gpu_ctx, bar):
    """Eight scans, three of them finished before the launch with arbitrary bytes in their state; then the scan pool's indirection: a
    list that solves a subset out of order (one of its scans finished), directly and by the two-stage route."""
    rng = np.random.RandomState(77)
    partials = cases.spread_rows(rng, 8, 9)
    states = [ref.make_state(q=cases.UNIT_QS[i % 2][1], t=(float(i), 0.5, -1.0), iterations=i) for i in range(8)]
    for i in (1, 4, 6):
        states[i] = ref.make_state(q=rng.randn(4), t=rng.randn(3), R=rng.randn(9), last_dx_norm=rng.rand(), last_eff=1234 + i, iterations=40 + i,
                                   converged=i % 2, done=1, status=i)
    tally = Tally()
    got, hb, _ = run_gn(api, gpu_ctx, partials, states, ref.P2LINE, bar, tally, tag="mixed")
    assert [int(d) for d in got["iterations"]] == [1, 41, 3, 4, 44, 6, 46, 8]
    for two_stage in (False, True):
        got, hb, _ = run_gn(api, gpu_ctx, partials, states, ref.P2LINE, bar, tally, scans=[7, 4, 2, 0], two_stage=two_stage, tag="listed %d" % two_stage)
        assert [int(d) for d in got["iterations"]] == [1, 41, 3, 3, 44, 5, 46, 8]
    assert tally.norms == 5 + 3 + 3


def test_bad_arguments_are_refused_and_nothing_is_written(api, gpu_ctx):
    L = api.lib()
    n, blocks = 4, 3
    p = cases.spread_rows(np.random.RandomState(1), n, blocks)
    st_in = pack_states(api, [ref.make_state() for _ in range(n)])
    st_out = np.zeros(n, dtype=api.SOLVE_STATE)
    st_out["iterations"] = -5
    hb = np.full((n, ref.HB_W), 3.5)
    hb_l = np.full((n, ref.LOAM_HB_W), 3.5)
    mins = np.array([10, 10], dtype=np.int32)

    def gn(ctx=gpu_ctx._h, partials=p.ctypes.data, n_scans=n, bps=blocks, method=ref.P2PLANE, scans=None, n_launch=0, s_in=st_in.ctypes.data, s_out=st_out.ctypes.data,
           hb_out=hb.ctypes.data):
        sc = None if scans is None else np.ascontiguousarray(scans, dtype=np.int32)
        return L.locgpu_debug_gn_solve(ctx, partials, n_scans, bps, method, 10, 1e-2, 20, 1, 0, None if sc is None else sc.ctypes.data, n_launch, s_in, s_out, hb_out)

    def loam(ctx=gpu_ctx._h, surf=p.ctypes.data, b_surf=blocks, edge=p.ctypes.data, b_edge=blocks, n_scans=n, m=mins.ctypes.data, s_in=st_in.ctypes.data,
             s_out=st_out.ctypes.data, hb_out=hb_l.ctypes.data):
        return L.locgpu_debug_loam_solve(ctx, surf, b_surf, edge, b_edge, n_scans, m, 1e-3, 20, 1, s_in, s_out, hb_out)

    bad = [gn(ctx=None), gn(partials=None), gn(s_in=None), gn(s_out=None), gn(hb_out=None), gn(n_scans=0), gn(n_scans=1025), gn(bps=0), gn(bps=4097),
           gn(method=-1), gn(method=6), gn(method=99), gn(scans=[0, 4], n_launch=2), gn(scans=[-1], n_launch=1), gn(scans=[1, 1], n_launch=2),
           gn(scans=[0], n_launch=0), gn(scans=[0, 1, 2, 3, 0], n_launch=5),
           loam(ctx=None), loam(surf=None, edge=None), loam(m=None), loam(s_in=None), loam(s_out=None), loam(hb_out=None), loam(n_scans=0), loam(n_scans=1025),
           loam(b_surf=0), loam(b_edge=4097)]
    assert bad == [-1] * len(bad), bad
    assert (st_out["iterations"] == -5).all() and (hb == 3.5).all() and (hb_l == 3.5).all()
    assert gn() == 0 and loam() == 0 and loam(surf=None, b_surf=0) == 0  # and the same arguments, well-formed, run
    assert (st_out["iterations"] == 1).all()


# -------------------------------------------------------------------------------------------------------------------------- LOAM
def run_loam(api, ctx, surf, edge, states, bar, tally, mins=(10, 7), eps=EPS_NEVER, max_it=20, do_update=True, tag=""):
    st_in = pack_states(api, states)
    hb_in = np.full((len(states), ref.LOAM_HB_W), -7.25)
    got, hb = ctx.debug_loam_solve(surf, edge, st_in, min_effective_pts=mins, eps=eps, max_iteration=max_it, do_update=do_update, hb=hb_in)
    steps = []
    for i, s in enumerate(states):
        want, want_hb, step = ref.loam_step(None if surf is None else ref.reduce_f64(surf[i]), None if edge is None else ref.reduce_f64(edge[i]), s, mins, eps,
                                            max_it, do_update)
        check_scan("%s scan %d" % (tag, i), st_in[i], got[i], hb[i], hb_in[i], want, want_hb, step, bar, tally)
        steps.append(step)
    return got, hb, steps


def test_loam_class_rules(api, gpu_ctx, bar):
    """Each class false alone by its count (min − 1; the two classes have different minima) and by its own det; both false; the count
    exactly at the minimum; H_edge = −H_surf — each regular, the sum the zero matrix; a finished scan. Status 3 whenever the surface class
    is false, 4 when only the edge class is; hb in the 46-double layout."""
    A, Bc, sing = cases.regular_case(0), cases.regular_case(1), cases.singular_cases()[2]
    row = lambda c, eff: ref.pack_row(c.H, c.B, eff)
    neg = ref.pack_row(-A.H, A.B, 30)
    table = [  # surface row, edge row, status, done, updated
        (row(A, 9), row(Bc, 50), 3, 1), (row(sing, 50), row(Bc, 50), 3, 1), (row(A, 50), row(Bc, 6), 4, 1), (row(A, 50), row(sing, 50), 4, 1),
        (row(A, 9), row(Bc, 6), 3, 1), (row(sing, 50), row(Bc, 6), 3, 1), (row(A, 10), row(Bc, 7), 0, 0), (row(A, 30), neg, 0, 0), (row(A, 50), row(Bc, 50), 0, 1),
    ]
    surf = np.stack([t[0] for t in table])[:, None, :]
    edge = np.stack([t[1] for t in table])[:, None, :]
    states = [ref.make_state(q=cases.UNIT_QS[i % 2][1], t=(1.0, 2.0, 3.0), last_dx_norm=0.5, iterations=2) for i in range(len(table))]
    states[8] = ref.make_state(q=(0.1, 0.2, 0.3, 0.4), iterations=9, done=1, status=4)
    tally = Tally()
    got, hb, steps = run_loam(api, gpu_ctx, surf, edge, states, bar, tally, tag="loam rules")
    st_in = pack_states(api, states)
    for i, (_, _, status, done) in enumerate(table[:8]):
        assert (got[i]["status"], got[i]["done"], got[i]["iterations"]) == (status, done, 3), i
        if i != 6:
            assert got[i]["q"].tobytes() == st_in[i]["q"].tobytes() and got[i]["t"].tobytes() == st_in[i]["t"].tobytes() and got[i]["last_dx_norm"] == 0.5, i
    assert steps[6].dx is not None and steps[7].lu.det == 0.0 and steps[7].dx is None
    assert (hb[7][:36] == 0.0).all() and list(hb[7][42:]) == [30.0, 30.0, 1.0, 1.0]
    assert list(hb[0][42:]) == [9.0, 50.0, 0.0, 1.0] and list(hb[3][42:]) == [50.0, 50.0, 1.0, 0.0] and list(hb[4][42:]) == [9.0, 6.0, 0.0, 0.0]
    assert got[6]["last_eff"] == 17 and tally.norms == 1


@pytest.mark.parametrize("off", ["surface", "edge"])
def test_loam_one_class_off(api, gpu_ctx, bar, off):
    """A class that is switched off is never evaluated: its effective_num is 0 and its ok is 1, whatever its minimum asks."""
    cs = (cases.regular_case(0), cases.pivot_cases()[1], cases.singular_cases()[0])
    on = np.stack([ref.pack_row(c.H, c.B, 50) for c in cs])[:, None, :]
    states = [ref.make_state(q=cases.UNIT_QS[1][1]) for _ in cs]
    tally = Tally()
    surf, edge = (None, on) if off == "surface" else (on, None)
    got, hb, steps = run_loam(api, gpu_ctx, surf, edge, states, bar, tally, mins=(10, 10), tag="loam %s off" % off)
    c_off = 0 if off == "surface" else 1
    for i in range(3):
        assert hb[i][42 + c_off] == 0.0 and hb[i][44 + c_off] == 1.0 and hb[i][43 - c_off] == 50.0
    assert [int(s) for s in got["status"]] == [0, 0, 4 if off == "surface" else 3] and tally.norms == 2


def test_loam_joint_solve(api, gpu_ctx, locref, bar):
    """Regular joint cases: the two classes' partials summed each in the documented order (3 and 9 rows), the sums added, and dx =
    lu6 of the summed H and B — t_out is the oracle's x[3:6] on that sum bit for bit; the update cases through H_surf + H_edge = I; the
    stop at |dx| = 2^-7 (strict) and the iteration limit."""
    rng = np.random.RandomState(31)
    cs = cases.pivot_cases()
    n = len(cs)
    surf = np.zeros((n, 3, ref.ACC_W))
    edge = np.zeros((n, 9, ref.ACC_W))
    for i, c in enumerate(cs):  # rows whose sum is near c.H, so that the summed matrices keep pivoting in many ways
        for rows, share in ((surf, 0.25), (edge, 0.75)):
            w = rng.rand(rows.shape[1])
            w = share * w / w.sum()
            for r in range(rows.shape[1]):
                rows[i, r] = ref.pack_row(w[r] * c.H, w[r] * c.B, 20)
    tally = Tally()
    got, hb, steps = run_loam(api, gpu_ctx, surf, edge, [ref.make_state() for _ in cs], bar, tally, tag="loam joint")
    pivots = set()
    for i in range(n):
        tot = ref.reduce_f64(surf[i]) + ref.reduce_f64(edge[i])
        H, B, _ = ref.unpack(tot)
        det, x = locref.lu6(np.array(H), np.array(B))
        assert det != 0.0 and np.array_equal(bits(got[i]["t"]), bits(0.0 + x[3:6])), i
        assert list(hb[i][42:]) == [60.0, 180.0, 1.0, 1.0]
        pivots |= set(enumerate(steps[i].lu.pivots))
    assert len(pivots) >= 15, sorted(pivots)
    # the update cases, H_surf = ¼ I, H_edge = ¾ I, the right-hand side on the edge class alone
    ucs = cases.update_cases()
    surf = np.stack([ref.pack_row(0.25 * np.eye(6), np.zeros(6), 50) for _ in ucs])[:, None, :]
    edge = np.stack([ref.pack_row(0.75 * np.eye(6), dx, 50) for _, _, _, dx in ucs])[:, None, :]
    run_loam(api, gpu_ctx, surf, edge, [ref.make_state(q=q, t=t) for _, q, t, _ in ucs], bar, tally, tag="loam update")
    # eps and the iteration limit
    surf = np.stack([ref.pack_row(0.5 * np.eye(6), [0, 0, 0, 0, 2.0 ** -8, 0], 50)] * 3)[:, None, :]
    states = [ref.make_state(), ref.make_state(iterations=19), ref.make_state(iterations=18)]
    for eps, open_after in ((2.0 ** -7, True), (math.nextafter(2.0 ** -7, 1.0), False)):
        got, hb, _ = run_loam(api, gpu_ctx, surf, surf, states, bar, tally, eps=eps, tag="loam eps %r" % eps)
        assert got[0]["last_dx_norm"] == 2.0 ** -7 and (got[0]["converged"], got[0]["done"]) == ((0, 0) if open_after else (1, 1))
        assert (got[1]["iterations"], got[1]["done"]) == (20, 1) and got[2]["done"] == (0 if open_after else 1)
    print("LOAM: last_dx_norm at most %d ulp from the restatement over %d updates; sin/cos q error %.3e (bar %.3e)" % (tally.norm_ulp, tally.norms, tally.trig_err, bar[0]))
