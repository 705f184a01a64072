"""The conditions of the designed collision cases of tests/ndt_table_cases.py, asserted from its numpy restatements, the host harness
tests/cpp/ndt_key_check.cpp (csrc/ndt_key.hpp and csrc/ndt_set_key.hpp compiled with a plain host compiler, with and without
AddressSanitizer + UBSan) and the oracle alone — nothing here needs a GPU. tests/test_gpu_ndt_tables.py runs the same cases on the
device; what it may assume about them is what passes here.

The per-point unit of that file's H/B bars is measured here too, the way test_ndt_hb_ref.py::test_per_point_unit_of_the_oracle does it:
the oracle's own worst per-point error against the long-double restatement on the designed queries, recorded in ndt_table_cases.UNIT."""
import os
import subprocess

import numpy as np
import pytest

import ndt_hb_cases as hb_cases
import ndt_hb_ref as ref
import ndt_table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loc_lib_amd", "csrc")
MAX_EXCLUDED = 0  # the designed points need no exclusion near the gate: not one (point, voxel) residual lies within GATE_REL of it
POSES = (tc.IDENTITY, tc.SMALL_POSE)


# ---------------------------------------------------------------------------------------------- the restatements are the headers'
def _lines():
    """(input lines of the harness, the restatement's (key, h32, h64) per line): every key of every case and its absent query keys."""
    lines, want = [], []

    def single(vox, cap):
        vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
        key = tc.ndt_pack(vox)
        for v, k, a, b in zip(vox.tolist(), key.tolist(), tc.ndt_hash32(key, cap).tolist(), tc.ndt_hash(key, cap).tolist()):
            lines.append("%d %d %d %d" % (v[0], v[1], v[2], cap))
            want.append((k, a, b))

    for name in tc.DIRECT_CASES:
        c = tc.direct_case(name)
        for vox in (c["kept"], c["dropped"], c["queries"]["absent"]):
            single(vox, c["cap"])
    for name in tc.INC_CASES:
        c = tc.inc_case(name)
        for live, cap in zip(c["live"], c["caps"]):
            single(live, cap)
        single(c["queries"]["absent"], c["caps"][-1])
    s = tc.set_case()
    for t in range(tc.SET_TARGETS):
        for u in range(tc.SET_TARGETS):  # every voxel under every target: the absent keys of the set are the other targets' voxels
            key = tc.ndt_set_pack(u, s["voxels"][t])
            for v, k, a, b in zip(s["voxels"][t].tolist(), key.tolist(), tc.ndt_hash32(key, s["cap"]).tolist(), tc.ndt_hash(key, s["cap"]).tolist()):
                lines.append("%d %d %d %d %d" % (v[0], v[1], v[2], u, s["cap"]))
                want.append((k, a, b))
    single([(-1048575, 1048575, 0), (1048575, -1048575, -1), (0, 0, 0)], 1 << 26)  # the edges of the range, the largest table
    return lines, want


def _harness(tmp_path, tag, flags):
    exe = str(tmp_path / ("ndt_key_" + tag))
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ndt_key_check.cpp"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def _compare(exe):
    lines, want = _lines()
    assert len(lines) > 1500
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert out[-1] == "ndt key harness ok" and len(out) == len(lines) + 1
    for line, got, w in zip(lines, out, want):
        f = got.split()
        assert f[0] == "key" and f[2] == "h32" and f[4] == "h64", got
        assert (int(f[1]), int(f[3]), int(f[5])) == w, (line, got, w)


def test_restated_packs_and_hashes_equal_the_host_harness(tmp_path):
    """ndt_pack, ndt_set_pack, ndt_hash32 and ndt_hash as numpy states them against the headers themselves, for every key of every case
    and every absent query key; the harness also checks the round trip at the range edges, linearity and the hashes' low bits."""
    exe, r = _harness(tmp_path, "plain", ["-O2"])
    assert r.returncode == 0, r.stderr[-2000:]
    _compare(exe)


def test_restated_packs_and_hashes_equal_the_host_harness_under_asan_ubsan(tmp_path):
    exe, r = _harness(tmp_path, "asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    _compare(exe)


def test_key_header_has_no_hip_and_the_kernels_header_takes_the_rules_from_it():
    key = open(os.path.join(CSRC, "ndt_key.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in key.splitlines())
    for word in ("hip/", "__global__", "__device__ ", "__forceinline__", "hipError"):
        assert word not in code.replace("__host__ __device__", ""), word
    kernels = open(os.path.join(CSRC, "ndt_kernels.hpp")).read()
    assert '#include "ndt_key.hpp"' in kernels
    for name in ("kNdtEmpty =", "kNdtBias =", "ndt_key_in_range(int", "ndt_pack(int", "ndt_hash(unsigned", "ndt_hash32(unsigned"):
        assert name in key and name not in kernels, name


def test_slot_read_back_is_declared_exported_bound_and_refuses_a_null_context(api):
    import ctypes
    import re
    L = api.lib()
    name = "locgpu_debug_ndt_slots"
    header = open(os.path.join(ROOT, "include", "locgpu.h")).read()
    m = re.search(r"LOCGPU_API\s+int\s+%s\s*\(([^;]*)\);" % name, header)
    assert m and hasattr(L, name) and name in api.ABI_SYMBOLS
    assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")) == 5
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % name, exported, re.M)
    above = header[:m.start()]
    comment = above[above.rindex("/*"):]
    for word in ("ndt_registration.cpp:87-148", ":150-183", "all ones", "-1", "NULL arrays", "locgpu_debug_batch_nn"):
        assert word in comment, word
    assert callable(api.Context.debug_ndt_slots)
    keys, vid, n = np.full(4, 7, np.uint64), np.full(4, 7, np.int32), ctypes.c_size_t(7)
    assert L.locgpu_debug_ndt_slots(None, keys.ctypes.data, vid.ctypes.data, 4, ctypes.byref(n)) == -1  # LOCGPU_ERR_INVALID, nothing touched
    assert (keys == 7).all() and (vid == 7).all() and n.value == 7


def test_capacity_rules():
    assert [tc.direct_capacity(r) for r in (0, 1, 32, 33, 48, 50, 64, 65, 120, 128, 129)] == [1024, 1024, 1024, 2048, 2048, 2048, 2048, 4096, 4096, 4096, 8192]
    assert tc.direct_capacity(1 << 21) == 1 << 26 and tc.direct_capacity((1 << 21) + 1) == 1 << 26 and tc.direct_capacity((1 << 25) + 1) == 1 << 27  # 32 x runs up to 2^26, then load 0.5
    assert [tc.inc_capacity(n) for n in (0, 1, 512, 513, 600, 1024, 1025)] == [1024, 1024, 1024, 2048, 2048, 2048, 4096]
    assert tc.inc_capacity(40, have=2048) == 2048  # grows only


def test_probe_simulation_on_a_hand_made_table():
    occ, disp = tc.probe_sim([6, 6, 7, 7, 2], 8)
    assert np.flatnonzero(occ).tolist() == [0, 1, 2, 6, 7]
    assert disp.tolist() == [3, 3, 2, 2, 0]  # last in: 6 → slot 1, 7 → slot 1; the key at 2 is alone
    assert tc.wrap_run(occ).tolist() == [6, 7, 0, 1, 2]
    assert tc.wrap_run(tc.probe_sim([3, 4], 8)[0]).tolist() == []
    assert tc.probe_sim([0, 0, 0], 8)[1].tolist() == [2, 2, 2]


# ---------------------------------------------------------------------------------------------- conditions of the design
def _run_facts(homes, cap):
    occ, disp = tc.probe_sim(homes, cap)
    run = tc.wrap_run(occ)
    inside = np.zeros(cap, bool)
    inside[run] = True
    return occ, disp, run, inside


def _query_kinds(q, present, slots_of, cap, inside):
    """The kinds of the queries recounted from the points alone: (points in present voxels per voxel, absent-in-run points in front of
    the wrap, behind it, points whose centre is absent and that have a present face neighbour in the run)."""
    present_t = {tuple(v): i for i, v in enumerate(np.asarray(present).tolist())}
    vox = tc.voxels_of(q["points"])
    per_voxel = np.zeros(len(present_t), dtype=np.int64)
    front = behind = neigh = 0
    homes = slots_of(vox)
    present_inside = {v for v, h in zip(present_t, slots_of(np.array(list(present_t)))) if inside[h]}
    for v, h in zip(vox.tolist(), homes.tolist()):
        if tuple(v) in present_t:
            per_voxel[present_t[tuple(v)]] += 1
            continue
        if inside[h]:
            front += h >= cap // 2
            behind += h < cap // 2
        if any(tuple(n) in present_inside for n in (np.array(v) + tc.NEARBY[1:]).tolist()):
            neigh += 1
    return per_voxel, front, behind, neigh


@pytest.mark.parametrize("name", tc.DIRECT_CASES)
def test_direct_case_is_what_it_claims(name):
    c = tc.direct_case(name)
    kept, cap = c["kept"], c["cap"]
    assert cap == tc.DIRECT_CAP == 2048 and len(kept) == 48 and len(c["cloud"]) == 48 * 8 + len(c["dropped"]) * 3
    counts = {}
    for v in map(tuple, tc.voxels_of(c["cloud"]).tolist()):
        counts[v] = counts.get(v, 0) + 1
    assert len(counts) == c["runs"] and sorted(v for v, n in counts.items() if n > tc.MIN_PTS) == sorted(map(tuple, kept.tolist()))
    assert sorted(v for v, n in counts.items() if n <= tc.MIN_PTS) == sorted(map(tuple, c["dropped"].tolist()))
    homes = tc.ndt_hash32(tc.ndt_pack(kept), cap)
    occ, disp, run, inside = _run_facts(homes, cap)
    print("%s: occupied run of %d slots from %d through the end to %d, largest worst-case displacement %d" % (name, len(run), run[0], run[-1], disp.max()))
    assert len(run) >= 3 and run[0] > run[-1]  # the run crosses cap − 1 → 0
    if name == "same_slot":
        assert (homes == cap - 1).sum() == 3 and disp.max() >= 2
        assert (homes < cap - tc.DIRECT_TAIL).sum() >= 40  # the rest is scattered
    else:
        assert (homes >= cap - tc.DIRECT_TAIL).all() and disp.max() >= 16 and len(run) == 48
        pairs = tc.face_adjacent_pairs(kept)
        assert len({i for p in pairs for i in p}) >= 8
    if name == "dropped_in_chain":
        dh = tc.ndt_hash32(tc.ndt_pack(c["dropped"]), cap)
        assert len(dh) == 2 and inside[dh].all() and c["runs"] == 50
        assert np.array_equal(c["kept"], tc.direct_case("end_chain")["kept"])
    q = c["queries"]
    per_voxel, front, behind, neigh = _query_kinds(q, kept, lambda v: tc.ndt_hash32(tc.ndt_pack(v), cap), cap, inside)
    print("%s: %d query points: %d in kept voxels, absent with a first slot inside the run %d in front of the wrap + %d behind, absent centre with a present face "
          "neighbour of the chain %d" % (name, len(q["points"]), per_voxel.sum(), front, behind, neigh))
    assert (per_voxel == 4).all() and front >= 8 and front + behind >= 32 and neigh >= 16 and len(q["points"]) < 400
    if name != "same_slot":
        dropped = tc.direct_case("dropped_in_chain")["dropped"]
        assert len(q["kind"]["dropped"]) >= 2 and tc._tuples(tc.voxels_of(q["points"][q["kind"]["dropped"]])) == tc._tuples(dropped)
    assert (q["points"] > 1.0).all()  # positive coordinates only


def test_set_case_is_what_it_claims():
    s = tc.set_case()
    cap = s["cap"]
    assert cap == tc.SET_CAP == 4096 and s["runs"] == 120 == sum(len(v) for v in s["voxels"])
    shared = tc._tuples(s["shared"])
    assert len(shared) >= 16 and shared <= tc._tuples(s["voxels"][0]) and shared <= tc._tuples(s["voxels"][2]) and not (shared & tc._tuples(s["voxels"][1]))
    for t in (0, 2):  # the shared triples land in one region under both targets
        assert (tc.ndt_hash32(tc.ndt_set_pack(t, s["shared"]), cap) >= cap - tc.SET_TAIL).all()
    assert (tc.ndt_hash32(s["keys"][1], cap) >= cap - tc.SET_TAIL).all()
    for t in range(3):
        assert len(tc._tuples(s["voxels"][t])) == len(s["voxels"][t]) == 40
        assert tc._tuples(tc.voxels_of(s["clouds"][t])) == tc._tuples(s["voxels"][t]) and len(s["clouds"][t]) == 40 * 8
        assert tc._tuples(tc.voxels_of(s["scans"][t])) == tc._tuples(np.vstack(s["voxels"]))  # one scan per target visits all of these coordinates
    a, b = s["clouds"][0], s["clouds"][2]
    assert not ({r.tobytes() for r in a} & {r.tobytes() for r in b})  # different points
    keys = np.concatenate(s["keys"])
    assert len(np.unique(keys)) == 120
    occ, disp, run, inside = _run_facts(tc.ndt_hash32(keys, cap), cap)
    print("set: occupied run of %d slots from %d through the end to %d, largest worst-case displacement %d" % (len(run), run[0], run[-1], disp.max()))
    assert run[0] > run[-1] and disp.max() >= 16 and len(run) == 120


@pytest.mark.parametrize("name", tc.INC_CASES)
def test_incremental_case_is_what_it_claims(name):
    c = tc.inc_case(name)
    sizes = [len(tc._tuples(tc.voxels_of(x))) for x in c["calls"]]
    if name == "growth":
        assert sizes == [500, 100] and [len(x) for x in c["calls"]] == [500, 100] and c["caps"] == [1024, 2048] and [len(x) for x in c["live"]] == [500, 600]
        assert (tc.ndt_hash(tc.ndt_pack(c["live"][-1]), 2048) >= 2048 - tc.INC_TAIL).sum() >= 24
    else:
        first, second = tc._tuples(tc.voxels_of(c["calls"][0])), tc._tuples(tc.voxels_of(c["calls"][1]))
        assert sizes[:2] == [40, 30] and len(first & second) == 10 and c["caps"] == [1024] * len(c["calls"])
        per_voxel = np.unique(tc.ndt_pack(tc.voxels_of(c["calls"][0])), return_counts=True)[1]
        assert per_voxel.min() == 1 and per_voxel.max() == 6
        assert (tc.ndt_hash(tc.ndt_pack(np.array(sorted(first | second))), 1024) >= 1024 - tc.INC_TAIL).all()
        if name == "lookup_chain":
            assert c["capacity"] == 100000 and [len(x) for x in c["live"]] == [40, 60]
        else:
            assert c["capacity"] == 50 and [len(x) for x in c["live"]] == [40, 49, 49] and sizes[2] == 5
            after2, back = tc._tuples(c["live"][1]), tc._tuples(tc.voxels_of(c["calls"][2]))
            assert len(first - after2) == 11 and back <= first - after2  # call 2 evicts chain members, call 3 returns to five of them
            assert back <= tc._tuples(c["live"][2])
    for i, (live, cap) in enumerate(zip(c["live"], c["caps"])):
        occ, disp, run, inside = _run_facts(tc.ndt_hash(tc.ndt_pack(live), cap), cap)
        print("%s after call %d: %d live voxels in %d slots, occupied run of %d slots from %d through the end to %d, largest worst-case displacement %d"
              % (name, i + 1, len(live), cap, len(run), run[0], run[-1], disp.max()))
        assert run[0] > run[-1] and disp.max() >= 16
    q = c["queries"]
    cap = c["caps"][-1]
    per_voxel, front, behind, neigh = _query_kinds(q, c["live"][-1], lambda v: tc.ndt_hash(tc.ndt_pack(v), cap), cap, inside)
    print("%s: %d query points: %d in %d live voxels, absent in the run %d + %d, absent centre with a live neighbour of the chain %d"
          % (name, len(q["points"]), per_voxel.sum(), (per_voxel > 0).sum(), front, behind, neigh))
    assert (per_voxel > 0).sum() >= 40 and front >= 8 and front + behind >= 32 and neigh >= 16 and len(q["points"]) < 400
    in_run = inside[tc.ndt_hash(tc.ndt_pack(c["live"][-1]), cap)]
    assert (per_voxel[in_run] > 0).sum() >= min(int(in_run.sum()), 30)  # the chain's own voxels are asked


# ---------------------------------------------------------------------------------------------- the oracle keeps the designed voxels
def _keys_equal(ndt, vox):
    keys = ndt.dump()[0]
    assert ndt.num_voxels() == len(keys) == len(vox)
    assert sorted(map(tuple, keys.tolist())) == sorted(map(tuple, np.asarray(vox).tolist()))


@pytest.fixture(scope="module")
def oracles(locref):
    out = {}
    for name in tc.DIRECT_CASES:
        for nearby in (1, 0):
            out[name, nearby] = tc.oracle_direct(locref, tc.direct_case(name)["cloud"], nearby)
    for name in tc.INC_CASES:
        out[name, 1] = tc.oracle_inc(locref, tc.inc_case(name))
    return out


def test_oracle_keeps_exactly_the_designed_voxels(locref, oracles):
    for name in tc.DIRECT_CASES:
        _keys_equal(oracles[name, 1], tc.direct_case(name)["kept"])
    s = tc.set_case()
    for t in range(tc.SET_TARGETS):
        _keys_equal(tc.oracle_direct(locref, s["clouds"][t]), s["voxels"][t])
    for name in tc.INC_CASES:
        c = tc.inc_case(name)
        ndt = locref.Ndt(method=2, res_outlier_th=tc.RES_TH, capacity=c["capacity"])
        for cloud, live in zip(c["calls"], c["live"]):
            ndt.set_target(cloud)
            _keys_equal(ndt, live)  # the LRU replay of the cases module is the oracle's, evictions included


def _evaluations():
    """(case, nearby type, method, weighted, queries) of every per-point evaluation the GPU test runs."""
    for name in tc.DIRECT_CASES:
        for nearby in (1, 0):
            yield name, nearby, 1, tc.direct_case(name)["queries"]
    for name in tc.INC_CASES:
        yield name, 1, 2, tc.inc_case(name)["queries"]


def test_no_residual_near_the_gate_and_the_neighbour_probes_hit(oracles):
    """Not one (point, voxel) residual of any query lies within GATE_REL of the gate (the cap on exclusions is 0), and every found voxel
    is accepted — so the per-point count of accepted pairs is the count of probes that hit, through the walk or not."""
    for name, nearby, method, q in _evaluations():
        for pose in POSES:
            pp = tc.restate(ref, oracles[name, nearby], q["points"], pose, nearby, weighted=method == 2)
            excluded = ref.near_gate(pp["res"], tc.RES_TH, hb_cases.GATE_REL)
            assert int(excluded.sum()) <= MAX_EXCLUDED
            found = ~np.isnan(pp["res"])
            assert np.array_equal(found, pp["accept"])
            hits0, hits_n = int(found[:, 0].sum()), int(found[:, 1:].sum())
            print("%s nearby %d pose %s: %d centre hits, %d neighbour hits, %d points without a voxel" % (name, nearby, "identity" if pose is tc.IDENTITY else "small", hits0, hits_n,
                                                                                                   int((pp["n_acc"] == 0).sum())))
            assert hits0 >= 80 and (pp["n_acc"] == 0).sum() >= (24 if nearby == 1 else 48)
            if nearby == 1:
                assert found[q["kind"]["neighbour"], 1:].any(axis=1).sum() >= 16  # centre absent, the neighbour found through the chain
            if pose is tc.IDENTITY:
                assert found[q["kind"]["present"], 0].all() and not found[q["kind"]["absent_front"], 0].any() and not found[q["kind"]["absent_behind"], 0].any()
                if "dropped" in q["kind"]:
                    assert not found[q["kind"]["dropped"], 0].any()


def test_per_point_unit_of_the_oracle_on_the_designed_queries(oracles):
    """The oracle's own worst per-point H and B error against ndt_hb_ref.per_point over the designed queries at both poses: the unit of
    the GPU test's per-point bar (ndt_hb_cases.BAR_FACTOR units). The recorded ndt_table_cases.UNIT may not be smaller than what is
    measured here."""
    worst = {1: [0.0, 0.0], 2: [0.0, 0.0]}
    for name, nearby, method, q in _evaluations():
        ndt, pts = oracles[name, nearby], q["points"]
        for pose in POSES:
            pp = tc.restate(ref, ndt, pts, pose, nearby, weighted=method == 2)
            rows = [ndt.hb(pts[i:i + 1], pose) for i in range(len(pts))]
            H = np.stack([r[1] for r in rows])
            B = np.stack([r[2] for r in rows])
            got = np.array([tc.accepted_pairs(method, r[1], r[3]) for r in rows])
            assert np.array_equal(got, pp["n_acc"])  # exactly, every point: nothing is excluded
            eh, eb = ref.point_errors(H, B, pp)
            print("%s nearby %d: oracle per point vs long double: H %.3e, B %.3e; points with an accepted voxel %d / %d, accepted pairs %d"
                  % (name, nearby, eh.max(), eb.max(), int((pp["n_acc"] > 0).sum()), len(pts), int(pp["n_acc"].sum())))
            w = worst[method]
            w[0], w[1] = max(w[0], eh.max()), max(w[1], eb.max())
    for method, (wh, wb) in worst.items():
        uh, ub = tc.UNIT[method]
        print("per-point unit on the designed queries, method %d: H %.3e, B %.3e (recorded %.2e, %.2e) → GPU bars %.2e, %.2e"
              % (method, wh, wb, uh, ub, hb_cases.BAR_FACTOR * uh, hb_cases.BAR_FACTOR * ub))
        assert wh <= uh and wb <= ub, (method, wh, wb)
