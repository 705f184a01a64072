"""The ICP accumulate kernels of csrc/icp_fit.hip — icp_plane_accum_kernel<0|1>, icp_line_accum_kernel, icp_point_accum_kernel,
icp_mapplane_accum_kernel — and the device fits of csrc/device_math.hpp (plane_null_vector, plane_null_vector_secular, line_direction)
PER POINT against the 60-digit restatement of tests/icp_hb_ref.py, and the solve kernel's iterates against the oracle's.

The measure. The error of a fitted singular vector grows with κ (plane: σ1/(σ3 − σ4) of the 5×4 matrix, line: σ1/(σ1 − σ2) of the
centred 5×3 matrix; 1 for P2P and the table look-up), and κ spans 70 … 5e5 over the inputs here: a per-point error is measured as
error / (u·κ), u = 2^-53, H relative to max|H_point|, B relative to max(|B_point|, sqrt(max|H_point|)). The bar is 8 units, a unit
being the ORACLE's own worst figure in that measure over the same inputs and never less than 1 (icp_hb_cases.UNIT, measured by
test_icp_hb_ref.py::test_per_point_unit_of_the_oracle):

    P2P        unit H 4.1, B 420  →  bar H 32.8, B 3360      P2Plane    unit H 27, B 1   →  bar H 216, B 8
    P2Line     unit H 11,  B 320  →  bar H 88,   B 2560      map-plane  unit H 85, B 52  →  bar H 680, B 416
    plane 4-vector of the table: unit 1 → bar 8

Aggregates (sums over a scan): test_gpu_parity._hb_close, H to 1e-9 of max|H|, B to 1e-8; integers exactly. Excluded from the
per-point comparison, each decided from the restatement alone: a gated quantity within 1e-9 (relative) of its gate, κ > 1e8, and
rank-deficient neighbourhoods (compared with the oracle by the aggregate bar: their vector is a convention shared with the checker).
Every test prints its worst observed figures next to its bars.

Observed on the MI355X (the whole file: 27 tests, 10 s), worst error / (u·κ) against the bar:

    per point, P2P                       H 4.04 / 32.8   B 413 / 3360    (B: the far patches, where e = p − qs cancels 500 m; the
    per point, P2Line                    H 6.30 / 88     B 316 / 2560     oracle's figure is the same, to three digits)
    per point, P2Plane (secular fit)     H 1.18 / 216    B 0.142 / 8     small world; designed kinds H ≤ 0.21
    per point, P2Plane (4-column fit)    H 9.88 / 216    B 0.186 / 8     the worst kind is collinear_1e-3, κ up to 5.2e5
    per point, map-plane                 H 15.7 / 680    B 38.4 / 416
    table rows, |dn4|                    0.0103 / 8 (small world, raw 2.4e-14), 0.0052 / 8 (designed); five orders of a cluster 0.0049
    rank-deficient rows against the oracle   2.1e-15 (bar 1e-9)
    effective_num and the accepted witness   equal on every compared point; nothing excluded but the 48 rank-deficient queries

    rungs (1, 2, 4, 8 points per thread): |dH| ≤ 1.4e-14 of max|H|, |dB| ≤ 1.2e-14, every entry bit-equal to entry 0
    iterates: |dH| ≤ 1.4e-14, |dB| ≤ 2.3e-13; the GPU's pose after k iterations within 7.6e-15 m / 0 rad of the oracle's k-th iterate

The plane kernel is closer to the restatement than the oracle is (unit 27: the oracle's 5×4 Jacobi SVD; the kernel's secular fit stays
below 1.2). Scratch builds with the Newton stop of the secular root at 1e-3, the bare hardware rsq in the secular fit's normalisation,
`>=` in the residual gates, line neighbours rounded through float, or one column of R transposed in plane_row each fail tests here
(the gates and the float rounding fail nothing in test_gpu_parity.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_hb_cases as cases
import icp_hb_ref as ref
import map_plane_ref
from conftest import pose_delta
from test_gpu_parity import HB_RTOL, _hb_close

pytestmark = pytest.mark.gpu

SETS = ["true_pose", "init_pose", "designed"]


@pytest.fixture(scope="module")
def inputs(locref, small_world):
    return cases.input_sets(locref, small_world)


@pytest.fixture(scope="module")
def restated(locref, inputs):
    """(input set, oracle method) → the restatement, made on first use and kept for the module."""
    cache = {}

    def get(name, method):
        if (name, method) not in cache:
            cache[name, method] = cases.restate(locref, inputs[name], method)
        return cache[name, method]
    return get


def _opts(api, method, inp=None, **kw):
    code = api.P2PLANE_MAP if method == cases.MAPPLANE else method
    if inp is not None:
        kw["approximate"] = int(inp["approximate"])
    return api.icp_opts(method=code, **kw)


def _row(row):
    """A 44-double row of icp_hb_batch as icp_hb returns it: (ok, H, B, effective_num)."""
    return bool(row[43]), row[:36].reshape(6, 6), row[36:42], int(row[42])


def _aggregate(tag, got, want, with_ok=True):
    ok_g, Hg, Bg, eff_g = got
    ok_o, Ho, Bo, eff_o = want
    scale = max(np.abs(Ho).max(), 1e-300)
    scale_b = max(np.abs(Bo).max(), np.abs(Ho).max() * 1e-6, 1e-300)
    dh, db = np.abs(Hg - Ho).max() / scale, np.abs(Bg - Bo).max() / scale_b
    print("%s: |dH|/max|H| %.2e (bar %.0e)  |dB|/scale %.2e (bar 1e-08)  effective_num %d / %d  ok %s / %s" % (tag, dh, HB_RTOL, db, eff_g, eff_o, ok_g, ok_o))
    assert np.isfinite(Hg).all() and np.isfinite(Bg).all()
    _hb_close(Hg, Bg, Ho, Bo)
    assert eff_g == eff_o
    if with_ok:
        assert ok_g == ok_o
    return dh, db


# ---------------------------------------------------------------------------------------------- 1. per point
@pytest.mark.parametrize("method", cases.ORACLE_METHODS)
@pytest.mark.parametrize("name", SETS)
def test_per_point_against_the_restatement(gpu_ctx, api, locref, inputs, restated, name, method):
    """A batch of one-point scans is a per-point dump of the accumulate kernel (icp_hb_cases.assert_per_point)."""
    inp, pp = inputs[name], restated(name, method)
    gpu_ctx.icp_set_target(inp["map"])
    hb = cases.one_point_rows(gpu_ctx, inp["scan"], inp["pose"], _opts(api, method, inp))
    cases.assert_per_point(name, method, hb, pp, inp)
    rd = np.flatnonzero(pp["rank_deficient"])
    if len(rd):  # the convention shared with the checker: those points as one scan, against the oracle, by the aggregate bar
        icp = locref.Icp(method=method, use_ann=inp["approximate"])
        icp.set_target(inp["map"])
        sub = np.ascontiguousarray(inp["scan"][rd])
        _aggregate("%s, the %d rank-deficient neighbourhoods" % (name, len(rd)), gpu_ctx.icp_hb(sub, inp["pose"], _opts(api, method, inp)), icp.hb(sub, inp["pose"]))


def test_per_point_with_the_four_column_plane_fit(tmp_path, inputs, restated):
    """LOCGPU_PLANE_FIT=0 (icp_plane_accum_kernel<0>: plane_null_vector alone) is read once per process: the P2Plane rows of a fresh
    child process, held to the same bars."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    blob = {}
    for name in SETS:
        inp = inputs[name]
        blob.update({"map_" + name: inp["map"], "scan_" + name: inp["scan"], "pose_" + name: inp["pose"], "approximate_" + name: int(inp["approximate"])})
    np.savez(fin, **blob)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_icp_hb_fit_case.py"), fin, fout],
                       env=dict(os.environ, LOCGPU_PLANE_FIT="0"), capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.load(fout)
    for name in SETS:
        cases.assert_per_point(name + " (4-column fit)", cases.P2PLANE, out[name], restated(name, cases.P2PLANE), inputs[name])


def test_point_gate_keeps_a_squared_distance_equal_to_the_threshold(gpu_ctx, api, locref):
    """`dis2 > max_nn_distance` refuses: e·e == 1.0 exactly is kept, the next float above is not. Dyadic coordinates under the identity
    pose, so e = p − qs is exact on every side. (The plane kernel's |dis| has no such case: its n4 is computed, never exact.)"""
    m = np.array([(16.0 * i + 0.25, 16.0 * j + 0.5, 0.75) for i in range(4) for j in range(4)], np.float32)
    at, above = [], []
    for k, p in enumerate(m):
        step = np.zeros(3, np.float32)
        step[k % 3] = 1.0 if k % 2 else -1.0
        q = p - step
        assert ((p.astype(np.float64) - q.astype(np.float64)) ** 2).sum() == 1.0
        at.append(q)
        away = np.array(q, copy=True)
        away[k % 3] = np.nextafter(q[k % 3], np.float32(-np.inf if step[k % 3] > 0 else np.inf))
        assert ((p.astype(np.float64) - away.astype(np.float64)) ** 2).sum() > 1.0
        above.append(away)
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    gpu_ctx.icp_set_target(m)
    icp = locref.Icp(method=cases.P2P)
    icp.set_target(m)
    opts = api.icp_opts(method=cases.P2P)
    for tag, s, eff in (("at the gate", np.stack(at), 16), ("one float above", np.stack(above), 0), ("both", np.stack(at + above), 16)):
        got, want = gpu_ctx.icp_hb(s, ident, opts), icp.hb(s, ident)
        pp = ref.per_point(ref.P2P, m, cases.neighbours(locref, locref.KdTree(m), s, ident, cases.P2P), s, ident)
        print("%s: effective_num GPU %d, oracle %d, restatement %d (want %d)" % (tag, got[3], want[3], pp["fitted"].sum(), eff))
        assert got[3] == want[3] == pp["fitted"].sum() == eff
        assert got[1][3, 3] == got[1][4, 4] == got[1][5, 5] == eff  # the −I3 block: a count
        _hb_close(got[1], got[2], want[1], want[2])
    hb = cases.one_point_rows(gpu_ctx, np.stack(at + above), ident, opts)
    assert hb[:, 42].tolist() == [1.0] * 16 + [0.0] * 16 and not hb[16:, :42].any()


# ---------------------------------------------------------------------------------------------- 2. the map-plane mode
@pytest.mark.parametrize("which", ["small", "designed"])
def test_plane_table_rows_against_the_exact_vectors(gpu_ctx, api, locref, inputs, which):
    """map_plane_fit_kernel calls plane_null_vector_secular and its fall-back like the plane kernel: every dumped row against the exact
    null vector of that point's exact 5-NN, up to sign, in |dn4| / (u·κ). Small world: 512 rows; designed map: all of them, where the five
    members of a cluster present one neighbourhood in five orders and must agree to the same bar."""
    inp = inputs["true_pose" if which == "small" else "designed"]
    m = np.asarray(inp["map"], dtype=np.float32)
    rows = np.arange(len(m))[::391][:512] if which == "small" else np.arange(len(m))
    nn = cases.exact_neighbourhoods(inp["tree"], m, rows)
    t = ref.plane_table(m, nn)
    gpu_ctx.icp_set_target(m)
    gpu_ctx.icp_build_map_planes()
    n4, valid = gpu_ctx.icp_map_planes_dump()
    near = (t["gates"] <= cases.GATE_REL).any(axis=1)
    keep = ~(near | ~(t["kappa"] <= cases.KAPPA_MAX) | t["rank_deficient"])
    assert keep.sum() >= 0.9 * len(rows) if which == "small" else keep.sum() == len(rows) - 5 * cases.PER_KIND
    assert np.array_equal(valid[rows][~near], t["valid"][~near])  # validity is exact away from the gate
    cmp_rows = keep & t["valid"]
    un = ref.in_units(ref.vector_errors(n4[rows], t["n4"], t["n4_lo"]), t["kappa"])
    bar = cases.BAR_FACTOR * cases.UNIT["n4"]
    raw = ref.vector_errors(n4[rows], t["n4"], t["n4_lo"])
    print("%s: %d rows compared, %d excluded; kappa %.3g … %.3g; |dn4| raw %.2e; in units of u·kappa: worst %.3g, median %.2g (bar %.3g = 8 x %.3g)"
          % (which, cmp_rows.sum(), (~keep).sum(), t["kappa"][cmp_rows].min(), t["kappa"][cmp_rows].max(), raw[cmp_rows].max(), un[cmp_rows].max(), np.median(un[cmp_rows]), bar, cases.UNIT["n4"]))
    for i in np.flatnonzero(cmp_rows & (un > bar))[:8]:
        print("    ABOVE THE BAR: row %d, kappa %.6g, %.3g units, n4 %s, neighbours:\n%s" % (rows[i], t["kappa"][i], un[i], n4[rows[i]].tolist(), m[nn[i]].tolist()))
    assert np.isfinite(n4[rows][valid[rows]]).all() and un[cmp_rows].max() <= bar
    if which == "designed":
        kind = np.repeat(cases.designed_map()[1], 5)
        for k, kname in enumerate(cases.KINDS):
            sel = cmp_rows & (kind == k)
            if sel.any():
                print("    %-16s kappa %.3g … %.3g  worst %.3g units" % (kname, t["kappa"][sel].min(), t["kappa"][sel].max(), un[sel].max()))
        # five orders of one neighbourhood
        assert (np.sort(nn.reshape(-1, 5, 5), axis=2) == np.sort(nn.reshape(-1, 5, 5), axis=2)[:, :1]).all()
        g = n4.reshape(-1, 5, 4)
        g = g * np.where((g * g[:, :1]).sum(axis=2, keepdims=True) < 0, -1.0, 1.0)
        spread = np.abs(g - g[:, :1]).max(axis=(1, 2)) / (ref.U * t["kappa"].reshape(-1, 5)[:, 0])
        ok_cluster = cmp_rows.reshape(-1, 5).all(axis=1)
        print("    the five orders of a cluster agree to %.3g units (bar %.3g)" % (spread[ok_cluster].max(), bar))
        assert spread[ok_cluster].max() <= bar
        # rank-deficient clusters: the rule's vector, against the oracle's fit, by the aggregate bar
        rd = np.flatnonzero(t["rank_deficient"])
        want = np.stack([locref.fit_plane(m[nn[i]].astype(np.float64))[1] for i in rd])
        d = np.minimum(np.abs(n4[rd] - want).max(axis=1), np.abs(n4[rd] + want).max(axis=1))
        print("    %d rank-deficient rows: |n4 - oracle| up to sign %.2e (bar %.0e)" % (len(rd), d.max(), HB_RTOL))
        assert len(rd) == 5 * cases.PER_KIND and d.max() <= HB_RTOL


@pytest.mark.parametrize("name", SETS)
def test_map_plane_rows_per_point(gpu_ctx, api, locref, inputs, name):
    """icp_mapplane_accum_kernel against the restatement fed with the DUMPED table: κ = 1, the table is data here."""
    inp = inputs[name]
    gpu_ctx.icp_set_target(inp["map"])
    gpu_ctx.icp_build_map_planes()
    planes = gpu_ctx.icp_map_planes_dump()
    pp = cases.restate(locref, inp, cases.MAPPLANE, planes=planes)
    assert pp["accepted"].sum() >= (cases.MIN_ACCEPTED if inp["kind"] is None else len(pp["accepted"]))
    hb = cases.one_point_rows(gpu_ctx, inp["scan"], inp["pose"], _opts(api, cases.MAPPLANE, inp))
    cases.assert_per_point(name, cases.MAPPLANE, hb, pp, inp)


# ---------------------------------------------------------------------------------------------- 3. points-per-thread rungs
@pytest.fixture(scope="module")
def scan8193(synth):
    s = synth.make_scan(3, subsample=8193, crop_half=36.0)
    assert len(s) == 8193  # 33 blocks of 256, the last one holding one point
    return s


@pytest.mark.parametrize("method", cases.ORACLE_METHODS + (cases.MAPPLANE,))
def test_points_per_thread_rungs(gpu_ctx, api, locref, small_world, inputs, scan8193, method):
    """33 blocks per entry x 1, 63, 125, 249 entries = 33, 2 079, 4 125, 8 217 blocks: icp_accum_split takes 1, 2, 4 and 8 points per
    thread (4 for the plane kernel), and the grid's last block runs partly past the scan. Every entry equals entry 0 bit for bit, and
    every rung the oracle."""
    pose, m = small_world["init_pose"], small_world["map"]
    gpu_ctx.icp_set_target(m)
    if method == cases.MAPPLANE:
        gpu_ctx.icp_build_map_planes()
        n4, valid = gpu_ctx.icp_map_planes_dump()
        want = map_plane_ref.hb(locref, inputs["true_pose"]["tree"], dict(n4=n4, valid=valid), scan8193, pose)
    else:
        icp = locref.Icp(method=method)
        icp.set_target(m)
        want = icp.hb(scan8193, pose)
    assert want[0] and want[3] > 4000
    for n_entries in (1, 63, 125, 249):
        b = gpu_ctx.batch_shared(scan8193, n_entries)
        try:
            hb = gpu_ctx.icp_hb_batch(b, np.stack([pose] * n_entries), _opts(api, method))
        finally:
            b.close()
        _aggregate("%s x%d" % (cases.NAMES[method], n_entries), _row(hb[0]), want)
        assert np.array_equal(hb[0, :36].reshape(6, 6), hb[0, :36].reshape(6, 6).T)
        differ = [e for e in range(1, n_entries) if hb[e].tobytes() != hb[0].tobytes()]
        assert not differ, differ[:8]


# ---------------------------------------------------------------------------------------------- 4. ragged and degenerate input
def _hostile(s):
    """s with NaN / ±inf / 1e30 rows mixed in."""
    h = np.array(s, copy=True)
    nan, inf = np.float32("nan"), np.float32("inf")
    for r, v in {3: (nan, 1, 2), 40: (1, nan, nan), 99: (inf, 0, 0), 100: (0, -inf, 1), 101: (inf, -inf, inf), 200: (1e30, 0, 0), 201: (0, -1e30, 1e30),
                 300: (nan, nan, nan), len(h) - 1: (-inf, 3e38, 1)}.items():
        h[r, :3] = v
    return h


@pytest.mark.parametrize("method", cases.ORACLE_METHODS + (cases.MAPPLANE,))
def test_ragged_and_degenerate_scans_in_one_batch(gpu_ctx, api, locref, small_world, inputs, method):
    """Scans of 0, 1, 255, 256 and 257 points, a scan with NaN / ±inf / 1e30 points mixed in, and a scan whose points all lie farther
    than every gate, in one batch; every row against the oracle's evaluation of that scan alone. The finite-point rule is P2P's (and the
    map-plane mode's): under P2Line and P2Plane a non-finite source point reaches the sums on either side, so there the rows must be
    non-finite in the same entries and close in the others."""
    s, pose, m = small_world["scan2k"], small_world["true_pose"], small_world["map"]
    far = np.array(s[1300:1500], copy=True)
    far[:, 2] += 1000.0
    scans = [s[:0], s[0:1], s[1:256], s[256:512], s[512:769], _hostile(s[770:1300]), far]
    gpu_ctx.icp_set_target(m)
    if method == cases.MAPPLANE:
        gpu_ctx.icp_build_map_planes()
        n4, valid = gpu_ctx.icp_map_planes_dump()
        oracle = lambda sc: map_plane_ref.hb(locref, inputs["true_pose"]["tree"], dict(n4=n4, valid=valid), sc, pose) if len(sc) else (False, np.zeros((6, 6)), np.zeros(6), 0)  # noqa: E731
    else:
        icp = locref.Icp(method=method)
        icp.set_target(m)
        oracle = lambda sc: icp.hb(sc, pose)  # noqa: E731
    b = gpu_ctx.batch(scans)
    try:
        hb = gpu_ctx.icp_hb_batch(b, np.stack([pose] * len(scans)), _opts(api, method))
    finally:
        b.close()
    for i, sc in enumerate(scans):
        tag = "%s scan %d (%d points)" % (cases.NAMES[method], i, len(sc))
        got, want = _row(hb[i]), oracle(sc)
        if i == 5 and method in (cases.P2LINE, cases.P2PLANE):
            fin = np.isfinite(want[1])
            print("%s: oracle H finite in %d of 36 entries, B in %d of 6; effective_num %d / %d" % (tag, fin.sum(), np.isfinite(want[2]).sum(), got[3], want[3]))
            assert np.array_equal(np.isfinite(got[1]), fin) and np.array_equal(np.isfinite(got[2]), np.isfinite(want[2]))
            assert got[3] == want[3] and got[0] == want[0]
            if fin.any():
                assert np.abs(got[1][fin] - want[1][fin]).max() <= HB_RTOL * np.abs(want[1][fin]).max()
            continue
        _aggregate(tag, got, want)
        if i in (0, 6):  # empty, all refused: exactly nothing (P2P counts accepted points, the others fitted ones)
            assert not got[1].any() and not got[2].any() and got[0] is False
            assert (got[3] == 0) == (i == 0 or method == cases.P2P)


# ---------------------------------------------------------------------------------------------- 5. every iterate of an alignment
@pytest.mark.parametrize("method", cases.ORACLE_METHODS)
def test_every_iterate_of_an_alignment(gpu_ctx, api, locref, small_world, method):
    """The oracle's trace rows (H, B, effective_num, ok of every iteration) at the oracle's own iterates, rebuilt from its dx; then the
    GPU's own pose after max_iteration = k against the oracle's k-th iterate: the pose and R the solve kernel writes between iterations."""
    m, scan, init = small_world["map"], small_world["scan10k"], small_world["init_pose"]
    gpu_ctx.icp_set_target(m)
    icp = locref.Icp(method=method)
    icp.set_target(m)
    ro = icp.align(scan, init, trace_cap=20)
    assert len(ro["trace"]) == ro["iters"] >= 3
    iterates = [np.array(init, dtype=np.float64)]
    worst = [0.0, 0.0]
    for it, row in enumerate(ro["trace"]):
        Ho, Bo, dx, eff_o, ok_o = row[:36].reshape(6, 6), row[36:42], row[42:48], int(row[48]), bool(row[49])
        got = gpu_ctx.icp_hb(scan, iterates[-1], api.icp_opts(method=method))
        dh, db = _aggregate("%s iteration %d" % (cases.NAMES[method], it), got, (ok_o, Ho, Bo, eff_o))
        worst = [max(worst[0], dh), max(worst[1], db)]
        assert np.array_equal(got[1], got[1].T)
        iterates.append(locref.apply_update(iterates[-1], dx) if ok_o else iterates[-1].copy())
    np.testing.assert_array_equal(iterates[-1], ro["pose"])  # the iterates rebuilt here are the oracle's
    worst_pose = [0.0, 0.0]
    for k in range(1, ro["iters"] + 1):
        pg, st = gpu_ctx.icp_align(scan, init, api.icp_opts(method=method, max_iteration=k))
        dt, dr = pose_delta(pg, iterates[k])
        worst_pose = [max(worst_pose[0], dt), max(worst_pose[1], dr)]
        assert st["iterations"] == k and dt < 1e-8 and dr < 1e-8, (k, dt, dr)
    print("%s: %d iterates, worst |dH| %.2e, |dB| %.2e; GPU pose after k iterations against the oracle's k-th iterate: %.2e m, %.2e rad (bar 1e-08)"
          % (cases.NAMES[method], ro["iters"], worst[0], worst[1], worst_pose[0], worst_pose[1]))
