"""The NDT voxel hash tables on designed collision chains (tests/ndt_table_cases.py; their conditions are asserted on the CPU by
tests/test_ndt_table_cases_ref.py): the direct table and the voxel set (ndt_claim_slot, ndt_hash32; read by ndt_accum_kernel and
ndt_fitness_accum_kernel under both key rules) and the incremental table (inc_table_kernel, ndt_hash; read by inc_lookup_kernel at
ingest and inc_accum_kernel at alignment). Dozens of voxels share the last few first slots of a table, so the chain runs through the
end of the table and a look-up walks up to about 50 (set: 120) slots, wrapping; absent voxels whose first slot lies in the chain are
refused only at its end.

What is compared, and how:
  the table itself   locgpu_debug_ndt_slots against the restated hashes and capacity rules: slot count, the keys present, the linear-
                     probing invariant of every key (which also proves the restated hash is the device's), the occupied set against the
                     simulation, the record indices — exactly;
  dumps              against locref.Ndt after every call at the bars of test_gpu_ndt_ingest_shapes.py (keys equal; direct mu bitwise, info
                     1e-12 of the voxel's largest entry; incremental mu 1e-9 absolute, info 1e-7); num_voxels equal after every call;
  accumulate kernels a batch of one-point scans: accepted (point, voxel) pairs per point exactly (under the cases' gate every probe that
                     hits is accepted), H and B per point to 8 units of ndt_table_cases.UNIT — the oracle's own worst per-point error
                     against the long-double restatement on these queries:
                         direct       unit H 4.4e-16, B 3.7e-14   →  bar H 3.52e-15, B 2.96e-13
                         incremental  unit H 7.6e-16, B 1.13e-12  →  bar H 6.08e-15, B 9.04e-12
                     and the whole query scan to test_gpu_parity._hb_close with effective_num and ok equal;
  fitness kernel     per point against ndt_score_ref: inliers and finite points exactly, score to 1e-9 relative;
  the set            per target against that target's oracle table alone; ndt_align_pairs bit for bit against ndt_align_batch on a context
                     holding that target alone (the contract of include/locgpu.h);
  determinism        three builds in one process: dumps byte-identical, the occupied set equal (the slot of a key may differ).

Observed on the MI355X (every test prints its figures next to its bars): longest walk to a present key read back from the device 47
slots (end_chain, dropped_in_chain), 2 (same_slot), 118 (set), 39 / 59 (lookup_chain after call 1 / 2), 48 (evict_from_chain), 36 / 33
(growth at 1 024 / 2 048 slots), every run crossing the end of the table; accepted pairs per point equal on every point; worst per-point
error direct H 4.32e-16, B 3.61e-14, incremental H 7.91e-16, B 1.13e-12 (about one unit each); whole scans 7.4e-16 of max|H| at the
worst; fitness scores within 5.8e-15 relative. Scratch builds with the walk deleted from ndt_accum_kernel, deleted from inc_lookup_kernel,
or cut off after four slots fail 7, 4 and 9 of the 33 tests here."""
import numpy as np
import pytest

import ndt_hb_cases as hb_cases
import ndt_hb_ref as ref
import ndt_score_ref as score_ref
import ndt_table_cases as tc
from test_gpu_ndt_ingest_shapes import _same_table
from test_gpu_ndt_pairs import _bits, _same_row
from test_gpu_parity import HB_RTOL, _hb_close

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-9  # the bar of test_gpu_ndt_fitness.py
POSES = (("identity", tc.IDENTITY), ("small pose", tc.SMALL_POSE))


def _direct_opts(api, nearby=1):
    return api.ndt_opts(nearby_type=nearby, res_outlier_th=tc.RES_TH, min_pts_in_voxel=tc.MIN_PTS)


def _inc_opts(api, case):
    return api.ndt_opts(method=api.INCREMENTAL_NDT, nearby_type=1, res_outlier_th=tc.RES_TH, capacity=case["capacity"])


def _start_inc(gpu_ctx, api):
    gpu_ctx.ndt_set_target(np.zeros((4, 3), np.float32), api.ndt_opts())  # a direct call drops an incremental set left by another test


@pytest.fixture(scope="module")
def set_ctx(api):
    api.lib()
    ctx = api.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------- the table itself
def _check_slots(tag, keys, vid, want_keys, slots_of, cap):
    """The read-back slot array against the design. Returns (slot of every present key, in the order of `want_keys`)."""
    want_keys = np.asarray(want_keys, dtype=np.uint64)
    assert len(keys) == len(vid) == cap, (tag, len(keys), cap)
    occ = keys != tc.EMPTY
    got = keys[occ]
    assert len(got) == len(want_keys) and len(np.unique(got)) == len(got), tag  # each once
    assert np.array_equal(np.sort(got), np.sort(want_keys)), tag
    assert (vid[~occ] == -1).all(), tag
    slot = np.flatnonzero(occ)
    home = slots_of(got)
    disp = (slot - home) & (cap - 1)
    for s, h, d in zip(slot.tolist(), home.tolist(), disp.tolist()):  # the linear-probing invariant
        path = (h + np.arange(d + 1)) & (cap - 1)
        assert occ[path].all(), (tag, "a free slot between the first slot %d and the slot %d of key %#x" % (h, s, int(keys[s])))
    sim, worst = tc.probe_sim(slots_of(want_keys), cap)
    assert np.array_equal(occ, sim), tag
    assert (disp <= worst[np.argsort(want_keys)][np.searchsorted(np.sort(want_keys), got)]).all(), tag  # no key beyond its worst case
    run = tc.wrap_run(occ)
    print("%s: %d keys in %d slots; the run through the end of the table read back: %d slots (%d … %d), longest walk to a present key %d slots"
          % (tag, len(got), cap, len(run), run[0] if len(run) else -1, run[-1] if len(run) else -1, int(disp.max())))
    assert len(run) >= 3 and run[0] > run[-1]
    at = {int(k): int(s) for k, s in zip(got.tolist(), slot.tolist())}
    return np.array([at[int(k)] for k in want_keys.tolist()])


@pytest.mark.parametrize("name", tc.DIRECT_CASES)
def test_direct_table_slots(gpu_ctx, api, name):
    c = tc.direct_case(name)
    gpu_ctx.ndt_set_target(c["cloud"], _direct_opts(api))
    info = gpu_ctx.ndt_target_info()
    assert info["capacity"] == c["cap"] == tc.direct_capacity(c["runs"]) and info["num_voxels"] == len(c["kept"])
    keys, vid = gpu_ctx.debug_ndt_slots()
    want = tc.ndt_pack(c["kept"])
    slot = _check_slots(name, keys, vid, want, lambda k: tc.ndt_hash32(k, c["cap"]), c["cap"])
    assert sorted(vid[slot].tolist()) == list(range(len(want)))  # a permutation of the records
    dk = gpu_ctx.ndt_dump()[0]
    assert np.array_equal(tc.ndt_pack(dk[vid[slot]]), want)  # record vid carries that slot's key
    again = gpu_ctx.debug_ndt_slots()
    assert again[0].tobytes() == keys.tobytes() and again[1].tobytes() == vid.tobytes()


def test_set_table_slots(set_ctx, api):
    s = tc.set_case()
    set_ctx.ndt_set_target_set(s["clouds"], _direct_opts(api))
    info = set_ctx.ndt_target_info()
    assert info["capacity"] == s["cap"] == tc.direct_capacity(s["runs"]) and info["num_voxels"] == s["runs"]
    assert set_ctx.ndt_set_info()["voxels"] == [len(v) for v in s["voxels"]]
    keys, vid = set_ctx.debug_ndt_slots()
    want = np.concatenate(s["keys"])
    slot = _check_slots("set", keys, vid, want, lambda k: tc.ndt_hash32(k, s["cap"]), s["cap"])
    assert sorted(vid[slot].tolist()) == list(range(len(want)))
    rec = np.concatenate([tc.ndt_set_pack(t, set_ctx.ndt_set_dump(t)[0]) for t in range(tc.SET_TARGETS)])  # the records in (target, key) order
    assert np.array_equal(rec[vid[slot]], want)


@pytest.mark.parametrize("name", tc.INC_CASES)
def test_incremental_table_slots_and_dumps_after_every_call(gpu_ctx, api, locref, name):
    """After every call: the rebuilt key → voxel table, num_voxels and the dump against the oracle. A look-up at ingest that misses a
    live voxel deep in the chain creates it a second time: num_voxels, the dump and the table's key list all show it."""
    c = tc.inc_case(name)
    _start_inc(gpu_ctx, api)
    opts = _inc_opts(api, c)
    ndt = locref.Ndt(method=locref.INCREMENTAL_NDT, res_outlier_th=tc.RES_TH, capacity=c["capacity"])
    for i, (cloud, live, cap) in enumerate(zip(c["calls"], c["live"], c["caps"])):
        gpu_ctx.ndt_set_target(cloud, opts)
        ndt.set_target(cloud)
        assert gpu_ctx.ndt_target_info()["num_voxels"] == ndt.num_voxels() == len(live), (name, i)
        assert _same_table(gpu_ctx, ndt, "incremental") == len(live)
        keys, vid = gpu_ctx.debug_ndt_slots()
        slot = _check_slots("%s after call %d" % (name, i + 1), keys, vid, tc.ndt_pack(live), lambda k: tc.ndt_hash(k, cap), cap)
        v = vid[slot]
        assert (v >= 0).all() and len(np.unique(v)) == len(v) == gpu_ctx.ndt_target_info()["num_voxels"], (name, i)


# ---------------------------------------------------------------------------------------------- dumps against the oracle
@pytest.mark.parametrize("name", tc.DIRECT_CASES)
def test_direct_dump_matches_oracle(gpu_ctx, api, locref, name):
    c = tc.direct_case(name)
    gpu_ctx.ndt_set_target(c["cloud"], _direct_opts(api))
    assert _same_table(gpu_ctx, tc.oracle_direct(locref, c["cloud"]), "direct") == len(c["kept"])


@pytest.fixture(scope="module")
def set_oracles(locref):
    s = tc.set_case()
    return [tc.oracle_direct(locref, s["clouds"][t]) for t in range(tc.SET_TARGETS)]


def test_set_dump_matches_one_oracle_per_target(set_ctx, api, set_oracles):
    s = tc.set_case()
    set_ctx.ndt_set_target_set(s["clouds"], _direct_opts(api))
    for t in range(tc.SET_TARGETS):
        kg, mug, ig = set_ctx.ndt_set_dump(t)
        ko, muo, io = set_oracles[t].dump()
        og, oo = np.lexsort(kg.T[::-1]), np.lexsort(ko.T[::-1])
        np.testing.assert_array_equal(kg[og], ko[oo])
        np.testing.assert_array_equal(mug[og], muo[oo])
        scale = np.abs(io[oo]).max(axis=(1, 2), keepdims=True)
        assert (np.abs(ig[og] - io[oo]) / scale).max() < 1e-12, t


# ---------------------------------------------------------------------------------------------- accumulate kernels, per point
def _per_point(gpu_ctx, tag, method, ndt, nearby, pts):
    """One-point scans through ndt_hb_batch at both poses against the restatement on the oracle's table; then the whole scan through
    ndt_hb against the oracle."""
    uh, ub = tc.UNIT[method]
    bar_h, bar_b = hb_cases.BAR_FACTOR * uh, hb_cases.BAR_FACTOR * ub
    b = gpu_ctx.batch([pts[i:i + 1] for i in range(len(pts))])
    try:
        for pose_name, pose in POSES:
            pp = tc.restate(ref, ndt, pts, pose, nearby, weighted=method == 2)
            assert not ref.near_gate(pp["res"], tc.RES_TH, hb_cases.GATE_REL).any()  # nothing is excluded
            hb = gpu_ctx.ndt_hb_batch(b, np.stack([pose] * len(pts)))
            assert np.isfinite(hb).all()
            H, B, eff = hb[:, :36].reshape(-1, 6, 6), hb[:, 36:42], hb[:, 42]
            got = np.array([tc.accepted_pairs(method, H[i], eff[i]) for i in range(len(pts))])
            wrong = np.flatnonzero(got != pp["n_acc"])
            print("%s, %s: accepted voxels per point differ on %d of %d points%s; %d pairs accepted, %d of them through a neighbour probe"
                  % (tag, pose_name, len(wrong), len(pts), (" (first: point %d, GPU %d, restatement %d)" % (wrong[0], got[wrong[0]], pp["n_acc"][wrong[0]])) if len(wrong) else "",
                     int(pp["n_acc"].sum()), int(pp["accept"][:, 1:].sum())))
            assert len(wrong) == 0
            if method == 1:
                assert (eff == 1).all()
            eh, eb = ref.point_errors(H, B, pp)
            print("%s, %s: worst per-point error H %.3e (bar %.2e = 8 x %.2e), B %.3e (bar %.2e = 8 x %.2e)" % (tag, pose_name, eh.max(), bar_h, uh, eb.max(), bar_b, ub))
            assert eh.max() <= bar_h and eb.max() <= bar_b
            assert np.array_equal(H, H.transpose(0, 2, 1))
            ok_g, Hg, Bg, eff_g = gpu_ctx.ndt_hb(pts, pose)
            ok_o, Ho, Bo, eff_o = ndt.hb(pts, pose)
            print("%s, %s: whole scan |dH|/max|H| %.2e (bar %.0e), |dB| %.2e, effective_num %d / %d, ok %s / %s"
                  % (tag, pose_name, np.abs(Hg - Ho).max() / np.abs(Ho).max(), HB_RTOL, np.abs(Bg - Bo).max(), eff_g, eff_o, ok_g, ok_o))
            _hb_close(Hg, Bg, Ho, Bo)
            assert eff_g == eff_o and ok_g == ok_o
            assert tc.accepted_pairs(method, Hg, eff_g) == tc.accepted_pairs(method, Ho, eff_o) == int(pp["n_acc"].sum())
    finally:
        b.close()


@pytest.mark.parametrize("nearby", [1, 0])
@pytest.mark.parametrize("name", tc.DIRECT_CASES)
def test_direct_accumulate_per_point(gpu_ctx, api, locref, name, nearby):
    c = tc.direct_case(name)
    gpu_ctx.ndt_set_target(c["cloud"], _direct_opts(api, nearby))
    _per_point(gpu_ctx, "%s %s" % (name, "NEARBY6" if nearby else "CENTER"), 1, tc.oracle_direct(locref, c["cloud"], nearby), nearby, c["queries"]["points"])


@pytest.mark.parametrize("name", tc.INC_CASES)
def test_incremental_accumulate_per_point(gpu_ctx, api, locref, name):
    c = tc.inc_case(name)
    _start_inc(gpu_ctx, api)
    for cloud in c["calls"]:
        gpu_ctx.ndt_set_target(cloud, _inc_opts(api, c))
    _per_point(gpu_ctx, name, 2, tc.oracle_inc(locref, c), 1, c["queries"]["points"])


# ---------------------------------------------------------------------------------------------- fitness kernel
def _score_per_point(locref, table, pts, pose, n_nearby):
    """Per point of `pts`: (inlier 0/1, its score = the smallest accepted residual, +inf without one) by ndt_score_ref."""
    res = score_ref.residuals(locref, table, pts, pose, 1.0, n_nearby)
    assert len(res) == len(pts) and score_ref.gate_margin(res, tc.RES_TH) > 1.0
    with np.errstate(invalid="ignore"):
        accept = ~(np.isnan(res) | (res > tc.RES_TH))
    return accept.any(axis=1).astype(np.int64), np.where(accept, res, np.inf).min(axis=1)


def _check_scores(tag, fit, inl, score):
    g_score = np.array([f.score for f in fit])
    g_inl = np.array([f.inliers for f in fit])
    g_fin = np.array([f.finite_points for f in fit])
    assert np.array_equal(g_inl, inl) and (g_fin == 1).all(), (tag, np.flatnonzero(g_inl != inl))
    hit = inl == 1
    assert np.isinf(g_score[~hit]).all() and (g_score[~hit] > 0).all(), tag
    rel = np.abs(g_score[hit] - score[hit]) / score[hit]
    print("%s: %d of %d points are inliers; worst relative score difference %.2e (bar %.0e)" % (tag, int(hit.sum()), len(inl), rel.max() if hit.any() else 0.0, SUM_RTOL))
    assert (np.abs(g_score[hit] - score[hit]) <= SUM_RTOL * score[hit]).all(), tag
    return g_score


@pytest.mark.parametrize("nearby", [1, 0])
@pytest.mark.parametrize("name", tc.DIRECT_CASES)
def test_direct_fitness_per_point(gpu_ctx, api, locref, name, nearby):
    c = tc.direct_case(name)
    pts = c["queries"]["points"]
    gpu_ctx.ndt_set_target(c["cloud"], _direct_opts(api, nearby))
    table = score_ref.Table(*tc.oracle_direct(locref, c["cloud"], nearby).dump())
    b = gpu_ctx.batch([pts[i:i + 1] for i in range(len(pts))])
    try:
        for pose_name, pose in POSES:
            inl, score = _score_per_point(locref, table, pts, pose, 7 if nearby else 1)
            assert 80 <= inl.sum() < len(pts)
            fit = gpu_ctx.ndt_fitness_batch(b, np.stack([pose] * len(pts)), raw=True)
            _check_scores("%s %s, %s" % (name, "NEARBY6" if nearby else "CENTER", pose_name), fit, inl, score)
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------- the set
def test_set_fitness_per_point_under_each_target(set_ctx, api, locref, set_oracles):
    """Every coordinate triple any target holds, visited under each of the three targets: a voxel of another target in the same chain is
    not a match."""
    s = tc.set_case()
    set_ctx.ndt_set_target_set(s["clouds"], _direct_opts(api))
    tables = [score_ref.Table(*o.dump()) for o in set_oracles]
    shared = tc._tuples(s["shared"])
    for k, pts in enumerate(s["scans"]):
        in_shared = np.array([tuple(v) in shared for v in tc.voxels_of(pts).tolist()])
        assert in_shared.sum() == 2 * len(shared)
        b = set_ctx.batch([pts[i:i + 1] for i in range(len(pts))])
        try:
            scores = []
            for t in range(tc.SET_TARGETS):
                inl, score = _score_per_point(locref, tables[t], pts, tc.IDENTITY, 7)
                fit = set_ctx.ndt_fitness_pairs(b, [t] * len(pts), np.stack([tc.IDENTITY] * len(pts)), raw=True)
                scores.append(_check_scores("set scan %d under target %d" % (k, t), fit, inl, score))
                own = np.array([tuple(v) in tc._tuples(s["voxels"][t]) for v in tc.voxels_of(pts).tolist()])
                assert inl[own].all() and inl.sum() >= 2 * len(s["voxels"][t])
            # a point in a voxel only targets 0 and 2 hold: both score it, differently (their points differ), and target 1 scores
            # nothing unless one of ITS voxels is a face neighbour (the restatement on target 1's table alone says which)
            inl1 = _score_per_point(locref, tables[1], pts, tc.IDENTITY, 7)[0]
            alone = in_shared & (inl1 == 0)
            assert alone.sum() >= len(shared)
            assert np.isinf(scores[1][alone]).all() and np.isfinite(scores[0][in_shared]).all() and np.isfinite(scores[2][in_shared]).all()
            assert (scores[0][in_shared] != scores[2][in_shared]).all()
        finally:
            b.close()


def test_set_align_pairs_equals_align_batch_on_each_target_alone(gpu_ctx, set_ctx, api):
    s = tc.set_case()
    opts = _direct_opts(api)
    set_ctx.ndt_set_target_set(s["clouds"], opts)
    bs, bo = set_ctx.batch(s["scans"]), gpu_ctx.batch(s["scans"])
    try:
        inits = np.tile(tc.IDENTITY, (3, 1))
        inits[:, 4:] += [[0.02, -0.01, 0.015], [-0.015, 0.02, 0.01], [0.01, 0.015, -0.02]]
        for target_of in ([0, 1, 2], [2, 0, 1]):
            poses, stats = set_ctx.ndt_align_pairs(bs, target_of, inits)
            for i, t in enumerate(target_of):
                gpu_ctx.ndt_set_target(s["clouds"][t], opts)
                po, so = gpu_ctx.ndt_align_batch(bo, inits)
                _same_row(poses[i], stats[i], po[i], so[i], (target_of, i))
                print("set scan %d against target %d: %d iterations, status %d, effective_num %d: bit-identical to the single-target context" %
                      (i, t, stats[i]["iterations"], stats[i]["status"], stats[i]["last_effective_num"]))
            assert any(not np.array_equal(_bits(poses[i]), _bits(inits[i])) for i in range(3))  # alignments that moved
    finally:
        bs.close()
        bo.close()


# ---------------------------------------------------------------------------------------------- determinism
def _dump_bytes(d):
    k, mu, info = d
    o = np.lexsort(k.T[::-1])
    return k[o].tobytes() + mu[o].tobytes() + info[o].tobytes()


@pytest.mark.parametrize("name", tc.DIRECT_CASES + ("set",))
def test_three_builds_give_the_same_bytes(gpu_ctx, set_ctx, api, name):
    """Which slot of the chain a key claims is a race; what the table holds is not."""
    first = None
    for rep in range(3):
        if name == "set":
            set_ctx.ndt_set_target_set(tc.set_case()["clouds"], _direct_opts(api))
            dump = b"".join(_dump_bytes(set_ctx.ndt_set_dump(t)) for t in range(tc.SET_TARGETS))
            keys = set_ctx.debug_ndt_slots()[0]
        else:
            gpu_ctx.ndt_set_target(tc.direct_case(name)["cloud"], _direct_opts(api))
            dump = _dump_bytes(gpu_ctx.ndt_dump())
            keys = gpu_ctx.debug_ndt_slots()[0]
        got = (dump, (keys != tc.EMPTY).tobytes(), np.sort(keys).tobytes())
        if first is None:
            first = got
        assert got == first, (name, rep)


# ---------------------------------------------------------------------------------------------- the read-back's own contract
def test_slot_read_back_counts_refuses_and_changes_nothing(gpu_ctx, api):
    import ctypes
    L = api.lib()
    n = ctypes.c_size_t(7)
    assert L.locgpu_debug_ndt_slots(None, None, None, 0, ctypes.byref(n)) == -1 and n.value == 7
    assert L.locgpu_debug_ndt_slots(gpu_ctx._h, None, None, 0, None) == -1
    fresh = api.Context(0)
    try:
        with pytest.raises(api.LocGpuError) as e:
            fresh.debug_ndt_slots()
        assert e.value.code == -3  # LOCGPU_ERR_NO_TARGET
    finally:
        fresh.close()
    c = tc.direct_case("end_chain")
    pts = c["queries"]["points"]
    gpu_ctx.ndt_set_target(c["cloud"], _direct_opts(api))
    before = gpu_ctx.ndt_align(pts, tc.SMALL_POSE)
    assert L.locgpu_debug_ndt_slots(gpu_ctx._h, None, None, 0, ctypes.byref(n)) == 0 and n.value == c["cap"]  # NULL arrays: the count only
    keys, vid = gpu_ctx.debug_ndt_slots()
    part_k, part_v = np.full(16, 5, np.uint64), np.full(16, 5, np.int32)
    assert L.locgpu_debug_ndt_slots(gpu_ctx._h, part_k.ctypes.data, part_v.ctypes.data, 10, ctypes.byref(n)) == 0 and n.value == c["cap"]
    assert np.array_equal(part_k[:10], keys[:10]) and np.array_equal(part_v[:10], vid[:10]) and (part_k[10:] == 5).all() and (part_v[10:] == 5).all()
    after = gpu_ctx.ndt_align(pts, tc.SMALL_POSE)
    assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1]
