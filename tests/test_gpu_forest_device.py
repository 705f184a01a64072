"""The ICP target's KD-trees built on the device (locgpu_icp_set_target_forest_device, locgpu_icp_set_target_cloud_device; DESIGN.md
§25). The reference is the library's own host build of the same points — locgpu_icp_set_target_forest_batch, locgpu_icp_set_target_cloud —
and the comparison is of BYTES, read back through locgpu_debug_tree_read after either build: slots, pads, sentinel leaves, leaf
slots; then of everything that reads the target (pairs alignment, k-NN, cloud alignment), bit for bit. The fixtures (tests/
forest_device_cases.py) have no degenerate split — tests/test_forest_device_abi.py checks that on the host — so a device call that
reports the device path really built these bytes itself."""
import numpy as np
import pytest

import forest_device_cases as cases
from loc_lib_amd.api import LocGpuError

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_DEPTH = -1, -5
SENTINEL = (0xC00000007F61B1E6, 0x7F61B1E67F61B1E6)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _state(ctx):
    """Everything a caller can see of the context's ICP target."""
    slots, leaves = ctx.debug_tree_read()
    try:
        forest = ctx.icp_forest_info()
    except LocGpuError:  # an ordinary target
        forest = None
    return dict(slots=slots, leaves=leaves, forest=forest, target=ctx.icp_target_info(), build=ctx.icp_device_build_info())


def _same_state(a, b, what, build=True):
    assert a["slots"].shape == b["slots"].shape and np.array_equal(a["slots"], b["slots"]), (what, int(np.sum(a["slots"] != b["slots"])) if a["slots"].shape == b["slots"].shape else "sizes")
    assert (a["leaves"] is None) == (b["leaves"] is None) and (a["leaves"] is None or np.array_equal(a["leaves"], b["leaves"])), what
    assert a["forest"] == b["forest"] and a["target"] == b["target"], (what, a["forest"], b["forest"], a["target"], b["target"])
    assert a["build"]["bounded"] == b["build"]["bounded"], what
    if build:
        assert a["build"] == b["build"], (what, a["build"], b["build"])


@pytest.fixture(scope="module")
def fctx(api):
    api.lib()
    ctx = api.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def big_forest(fctx, synth):
    """Computed once: the forest of all size cases and special trees, built by the host call and by the device call from one batch."""
    targets = cases.forest_targets(synth)
    clouds = [c for _, c in targets]
    b = fctx.batch(clouds)
    fctx.icp_set_target_forest_batch(b)
    host = _state(fctx)
    fctx.icp_set_target_forest_device(b)
    dev = _state(fctx)
    yield dict(names=[n for n, _ in targets], clouds=clouds, batch=b, host=host, dev=dev)
    b.close()


def test_thresholds_are_the_fixtures(fctx, big_forest):
    info = big_forest["dev"]["build"]
    assert (info["tile"], info["lane_len"]) == (cases.TILE, cases.LANE_LEN), info
    assert info["threads"] % 64 == 0


def test_forest_bytes_equal_the_host_build(fctx, big_forest, api):
    """Every tree of the forest — 1 … 20 000 points, both parities, around 64 and around both thresholds, the line, the tie, the offset
    cloud, the subnormal cloud — byte for byte the host build, pads and sentinel leaves included; the same forest and target infos; the
    report says the device built it."""
    host, dev, clouds = big_forest["host"], big_forest["dev"], big_forest["clouds"]
    assert dev["build"]["path"] == api.BUILD_PATH_DEVICE and dev["build"]["first_degenerate"] == -1 and dev["build"]["kind"] == 1, dev["build"]
    assert dev["build"]["levels"] == max(dev["forest"]["depth"]) - 1
    assert dev["forest"]["n_targets"] == len(clouds) and dev["forest"]["leaves"] == [len(c) for c in clouds]
    # per tree first, so that a failure names the tree: bases are even, ascending, 3n − 1 slots and a sentinel leaf each
    at = 0
    for name, c in zip(big_forest["names"], clouds):
        at += at & 1
        seg = 3 * len(c) - 1
        h, d = host["slots"][at:at + seg + 2], dev["slots"][at:at + seg + 2]
        assert np.array_equal(h, d), (name, len(c), int(np.sum(h != d)), int(np.argmax(h != d)))
        assert tuple(int(v) for v in d[seg:]) == SENTINEL, name
        at += seg + 2
    assert at == len(dev["slots"])
    _same_state(host, dev, "forest", build=False)
    assert dev["build"]["bounded"] is True


def test_align_pairs_after_the_device_build(fctx, api, synth):
    """locgpu_icp_align_pairs (P2PLANE, six scans against five of them, a local map and a five-point target) after the device build:
    poses and stats bit for bit those after the host build of the same batch."""
    world = cases.pair_world(synth)
    opts = api.icp_opts(method=api.P2PLANE)
    bt, bs = fctx.batch(world["targets"]), fctx.batch(world["scans"])
    try:
        fctx.icp_set_target_forest_batch(bt)
        host = _state(fctx)
        want_p, want_s = fctx.icp_align_pairs(bs, world["target_of"], None, opts)
        fctx.icp_set_target_forest_device(bt)
        dev = _state(fctx)
        assert dev["build"]["path"] == api.BUILD_PATH_DEVICE
        _same_state(host, dev, "pairs forest", build=False)
        got_p, got_s = fctx.icp_align_pairs(bs, world["target_of"], None, opts)
        assert np.array_equal(_bits(got_p), _bits(want_p))
        for i, (g, w) in enumerate(zip(got_s, want_s)):
            for key in ("iterations", "converged", "status", "last_effective_num"):
                assert g[key] == w[key], (i, key, g, w)
            assert np.array_equal(_bits([g["last_dx_norm"]]), _bits([w["last_dx_norm"]])), (i, g, w)
        assert sum(s["iterations"] > 1 for s in got_s) >= 4
    finally:
        bt.close()
        bs.close()


def test_duplicate_point_takes_the_host_path(fctx, api):
    scans = cases.with_duplicate()
    b = fctx.batch(scans)
    try:
        fctx.icp_set_target_forest_batch(b)
        host = _state(fctx)
        fctx.icp_set_target_forest_device(b)
        dev = _state(fctx)
        assert dev["build"]["path"] == api.BUILD_PATH_HOST and dev["build"]["first_degenerate"] == 1 and dev["build"]["kind"] == 1, dev["build"]
        _same_state(host, dev, "duplicate", build=False)
        assert dev["target"]["num_leaves"] == sum(len(s) for s in scans) - 1
    finally:
        b.close()


def test_huge_coordinate_gives_the_host_paths_bounded(fctx, api):
    """One coordinate of 1e19: whichever path the call takes, the bytes and the `bounded` outcome are the host call's (not bounded)."""
    b = fctx.batch(cases.with_huge())
    try:
        fctx.icp_set_target_forest_batch(b)
        host = _state(fctx)
        fctx.icp_set_target_forest_device(b)
        dev = _state(fctx)
        print("1e19 case: path", dev["build"]["path"])
        _same_state(host, dev, "1e19", build=False)
        assert host["build"]["bounded"] is False and dev["build"]["bounded"] is False
        assert dev["build"]["path"] == api.BUILD_PATH_DEVICE  # the fixture has no degenerate split (test_forest_device_abi.py)
    finally:
        b.close()


def test_refusals_leave_the_context_as_it_was(fctx, api, synth, big_forest):
    fctx.icp_set_target_forest_device(big_forest["batch"])
    before = _state(fctx)
    _same_state(big_forest["dev"], before, "rebuilt")
    a, c = cases.with_duplicate()[0], cases.with_duplicate()[2]
    other = api.Context(0)
    made = []
    try:
        def refused(batch, code, word):
            with pytest.raises(api.LocGpuError) as e:
                fctx.icp_set_target_forest_device(batch)
            assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
            _same_state(before, _state(fctx), word)

        empty = fctx.batch([a, np.zeros((0, 3), np.float32), c]); made.append(empty)
        refused(empty, ERR_INVALID, "target 1")
        foreign = other.batch([a, c]); made.append(foreign)
        refused(foreign, ERR_INVALID, "another context")
        sharded = fctx.batch([a, c], first=0, n_total=2); made.append(sharded)
        refused(sharded, ERR_INVALID, "sharded")
        shared = fctx.batch_shared(a, 3); made.append(shared)
        refused(shared, ERR_INVALID, "shared-source")
        # a tree deeper than the 64-entry traversal stack, second of three: the host call refuses it, and so does the device call
        deep = fctx.batch([a, cases.deep_chain(), c]); made.append(deep)
        with pytest.raises(api.LocGpuError) as e:
            fctx.icp_set_target_forest_batch(deep)
        assert e.value.code == ERR_DEPTH
        refused(deep, ERR_DEPTH, "target 1")
        deep_cloud = api.Cloud(fctx, np.concatenate([cases.deep_chain(), np.zeros((72, 1), np.float32)], axis=1))
        with pytest.raises(api.LocGpuError) as e:
            fctx.icp_set_target_cloud_device(deep_cloud)
        assert e.value.code == ERR_DEPTH
        _same_state(before, _state(fctx), "deep cloud")
        with pytest.raises(api.LocGpuError) as e:
            fctx.icp_set_target_cloud_device(api.Cloud(other, np.zeros((4, 4), np.float32)))
        assert e.value.code == ERR_INVALID
        _same_state(before, _state(fctx), "foreign cloud")
    finally:
        for b in made:
            b.close()
        other.close()


@pytest.mark.parametrize("which", [0, 1])
def test_single_cloud(fctx, gpu_ctx, api, synth, big_forest, which):
    """A resident cloud of 257 / 20 000 points as an ordinary target: slots, sentinel leaf and leaf slots equal locgpu_icp_set_target_cloud's,
    and so do the k-NN lists and the pose of a cloud alignment, bit for bit — on a context that held a forest a moment ago."""
    pts = cases.single_clouds(synth)[which]
    xyzi = np.zeros((len(pts), 4), np.float32)
    xyzi[:, :3] = pts
    rng = np.random.default_rng(5 + which)
    q = (pts[rng.integers(0, len(pts), 300)] + rng.normal(0, 0.3, (300, 3))).astype(np.float32)
    src = np.zeros((min(len(pts), 1500), 4), np.float32)
    src[:, :3] = pts[:len(src)] + np.float32(0.05)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    opts = api.icp_opts(method=api.P2PLANE)
    k = 5

    def readers(ctx):
        cloud = api.Cloud(ctx, src)
        pose, st = ctx.icp_align_cloud(cloud, ident, opts)
        return ctx.knn(q, k=k, approximate=True, alpha=0.1), ctx.knn(q, k=k, approximate=False), pose, st

    gpu_ctx.icp_set_target_cloud(api.Cloud(gpu_ctx, xyzi))
    host = _state(gpu_ctx)
    want = readers(gpu_ctx)
    fctx.icp_set_target_forest_device(big_forest["batch"])  # the context holds a forest …
    with pytest.raises(api.LocGpuError):
        fctx.knn(q, k=k)
    fctx.icp_set_target_cloud_device(api.Cloud(fctx, xyzi))  # … and is ordinary again
    dev = _state(fctx)
    assert dev["build"]["path"] == api.BUILD_PATH_DEVICE and dev["build"]["kind"] == 2, dev["build"]
    assert dev["forest"] is None and dev["leaves"] is not None and len(dev["leaves"]) == len(pts)
    _same_state(host, dev, "single cloud", build=False)
    assert tuple(int(v) for v in dev["slots"][-2:]) == SENTINEL
    got = readers(fctx)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[2]), _bits(want[2])) and got[3] == want[3], (got[2], want[2], got[3], want[3])
    assert got[3]["iterations"] >= 1
