"""Edge shapes of the NDT ingest front (csrc/ndt_ingest.hip), which builds the direct and the incremental voxel table alike: cloud
sizes around the 256-thread block of its key / head / runs kernels, one run, as many runs as points, a call that adds no voxel and one
that adds only new ones, and a point outside the ±2^20-voxel key range. The block sizes come twice: in the sparse ±4 m cube and in
a dense 3 m cube in which the direct table keeps its voxels too.

Every case compares ndt_dump() and num_voxels with the oracle's (locref.Ndt), an empty table included. Bars: those of
test_gpu_parity's test_ndt_voxel_table_matches_oracle and test_incremental_ndt_matches_oracle — the keys equal for both methods; direct:
μ bitwise, info to 1e-12 of the voxel's largest entry; incremental: μ to 1e-9 absolute, info to 1e-7 of the voxel's largest entry.

A cloud with a point outside the key range, as observed on the build before the front was shared and unchanged since:
    direct       the call fails with LOCGPU_ERR_INVALID (-1) and the context has no NDT target afterwards (ndt_target_info fails with
                 LOCGPU_ERR_NO_TARGET, -3): the previous table does not survive, ndt_build starts by dropping it.
    incremental  the call fails with LOCGPU_ERR_INVALID (-1) after ingesting every other point of the cloud ("it was skipped"): the
                 voxel set is the oracle's for the previous clouds plus this cloud without that point.
For both the next good call works. All clouds come from a seeded RandomState; voxel size 1.0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ["direct", "incremental"]
ERR_INVALID, ERR_NO_TARGET = -1, -3
FAR = 2.0e6  # metres = voxels: beyond the 2^20 = 1 048 576 voxels of the key range


def _pair(gpu_ctx, api, locref, method):
    """(options of the product, a fresh oracle) for a method; the product's voxel set starts empty."""
    gpu_ctx.ndt_set_target(np.zeros((4, 3), np.float32), api.ndt_opts())  # a direct call drops an incremental set left by another test
    if method == "direct":
        return api.ndt_opts(), locref.Ndt()
    return api.ndt_opts(method=api.INCREMENTAL_NDT), locref.Ndt(method=locref.INCREMENTAL_NDT)


def _same_table(gpu_ctx, ndt, method):
    kg, mug, ig = gpu_ctx.ndt_dump()
    ko, muo, io = ndt.dump()
    assert len(kg) == len(ko) == gpu_ctx.ndt_target_info()["num_voxels"] == ndt.num_voxels()
    og, oo = np.lexsort(kg.T[::-1]), np.lexsort(ko.T[::-1])
    np.testing.assert_array_equal(kg[og], ko[oo])
    if len(ko) == 0:
        return 0
    if method == "direct":
        np.testing.assert_array_equal(mug[og], muo[oo])
    else:
        np.testing.assert_allclose(mug[og], muo[oo], rtol=0, atol=1e-9)
    scale = np.abs(io[oo]).max(axis=(1, 2), keepdims=True)
    assert (np.abs(ig[og] - io[oo]) / scale).max() < (1e-12 if method == "direct" else 1e-7)
    return len(ko)


def _ingest_both(gpu_ctx, ndt, opts, cloud, method):
    gpu_ctx.ndt_set_target(cloud, opts)
    ndt.set_target(cloud)
    return _same_table(gpu_ctx, ndt, method)


def _cube(rng, n):
    return (rng.rand(n, 3) * 8.0 - 4.0).astype(np.float32)


def _lattice(rng, n):
    """n points, each in a voxel of its own: cell centres of a 1 m lattice, half of them at negative x (keys truncate toward zero,
    so the cells either side of 0 are kept apart)."""
    cells = rng.permutation(7 * 7 * 7)[:n]
    p = np.stack([cells // 49, (cells // 7) % 7, cells % 7], axis=1).astype(np.float64) + 0.5
    p[1::2, 0] = -(p[1::2, 0] + 1.0)
    return p.astype(np.float32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_sizes_around_the_block(gpu_ctx, api, locref, method, n):
    """The last block of the front's kernels holds 1, 255, 0, 1, 1 points."""
    opts, ndt = _pair(gpu_ctx, api, locref, method)
    kept = _ingest_both(gpu_ctx, ndt, opts, _cube(np.random.RandomState(100 + n), n), method)
    if n >= 255 and method == "incremental":
        assert kept > 100  # 343 voxels in the cube (the cells at 0 are double width), n >= 255 points: about 180 of them are touched


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_sizes_around_the_block_dense(gpu_ctx, api, locref, method, n):
    """The same sizes with the points in the 27 unit voxels of [0, 3) m³. In the ±4 m cube above a voxel holds less than one point on
    average and the direct table, which wants more than min_pts_in_voxel = 3, keeps only the few double-width cells at 0; here a voxel
    holds n / 27 >= 9.4 points on average, so the direct table with its bitwise μ bar is as full as the incremental one and a point lost
    in the last block changes a kept voxel. Floor: a Poisson count of mean 9.4 is 3 or less with probability 0.015, i.e. 0.4 voxels of
    27 are expected to be dropped; 20 kept leaves room for seven."""
    opts, ndt = _pair(gpu_ctx, api, locref, method)
    cloud = (np.random.RandomState(200 + n).rand(n, 3) * 3.0).astype(np.float32)
    assert _ingest_both(gpu_ctx, ndt, opts, cloud, method) >= 20


@pytest.mark.parametrize("method", METHODS)
def test_one_run(gpu_ctx, api, locref, method):
    """All points in one voxel: ustart[1] = n is the only boundary."""
    opts, ndt = _pair(gpu_ctx, api, locref, method)
    cloud = (np.random.RandomState(7).rand(300, 3) * 0.9 + 2.05).astype(np.float32)
    assert _ingest_both(gpu_ctx, ndt, opts, cloud, method) == 1


@pytest.mark.parametrize("method", METHODS)
def test_as_many_runs_as_points(gpu_ctx, api, locref, method):
    """Every point in a voxel of its own: the per-run arrays are as long as the per-point ones. The direct table keeps none of them
    (a voxel needs more than min_pts_in_voxel points), the incremental one all."""
    opts, ndt = _pair(gpu_ctx, api, locref, method)
    kept = _ingest_both(gpu_ctx, ndt, opts, _lattice(np.random.RandomState(8), 300), method)
    assert kept == (0 if method == "direct" else 300)


def test_incremental_no_new_then_only_new(gpu_ctx, api, locref):
    """A second call that touches only voxels that exist (new = 0), a third that touches only new ones (new = runs)."""
    opts, ndt = _pair(gpu_ctx, api, locref, "incremental")
    first = _cube(np.random.RandomState(9), 513)
    n1 = _ingest_both(gpu_ctx, ndt, opts, first, "incremental")
    assert _ingest_both(gpu_ctx, ndt, opts, first[::2], "incremental") == n1
    n3 = _ingest_both(gpu_ctx, ndt, opts, first[::3] + np.float32(20.0), "incremental")
    assert n3 > n1


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("where", ["first", "last"])
def test_point_outside_the_key_range(gpu_ctx, api, locref, method, where):
    """See the module docstring for what a refused cloud leaves behind; the incremental call is the one whose last run is the run of
    skipped points."""
    opts, ndt = _pair(gpu_ctx, api, locref, method)
    rng = np.random.RandomState(10)
    _ingest_both(gpu_ctx, ndt, opts, _cube(rng, 257), method)
    good = _cube(rng, 256)
    far = np.array([[FAR, 0.5, 0.5]], np.float32)
    with pytest.raises(api.LocGpuError) as err:
        gpu_ctx.ndt_set_target(np.concatenate([far, good] if where == "first" else [good, far]), opts)
    assert err.value.code == ERR_INVALID
    if method == "direct":
        with pytest.raises(api.LocGpuError) as err:
            gpu_ctx.ndt_target_info()
        assert err.value.code == ERR_NO_TARGET
    else:
        ndt.set_target(good)
        _same_table(gpu_ctx, ndt, method)
    _ingest_both(gpu_ctx, ndt, opts, _cube(rng, 300) + np.float32(1.0), method)
