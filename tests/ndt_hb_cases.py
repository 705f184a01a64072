"""Inputs shared by tests/test_ndt_hb_ref.py (CPU) and tests/test_gpu_ndt_hb.py (GPU): the NDT targets of the small world, the
per-point sample and the bars. Built from the existing fixtures only."""
import numpy as np

import ndt_hb_ref as ref

# name → (oracle / product method: 1 direct, 2 incremental; nearby type: 1 NEARBY6, 0 CENTER; res_outlier_th)
CASES = {
    "direct_nearby6": (1, 1, 20.0),
    "direct_nearby6_th5": (1, 1, 5.0),
    "direct_center": (1, 0, 20.0),
    "inc_th5": (2, 1, 5.0),
}

# The per-point unit: the ORACLE's worst per-point error against the long-double restatement over the 512-point sample, per method
# (the direct cases together; the info-weighted incremental sums carry the voxels' conditioning and are looser), measured and printed by
# test_ndt_hb_ref.py::test_per_point_unit_of_the_oracle, which also checks that these figures are not below what it measures. H relative to
# max|H_point|, B relative to max(|B_point|, sqrt(max|H_point|)). The GPU's per-point bar is 8 units.
UNIT = {1: (4.9e-16, 1.9e-14), 2: (9.0e-16, 1.18e-13)}  # method → (H, B)
BAR_FACTOR = 8.0
GATE_REL = 1e-9      # a pair this close (relative) to res_outlier_th may fall either side of the gate: its point is excluded from exact counts
MAX_EXCLUDED = 0.01  # share of the sample that may be excluded that way


def inc_clouds(locref, synth, small_world):
    """The three clouds test_incremental_ndt_matches_oracle feeds the incremental target."""
    def world_scan(sid, n):
        s = synth.make_scan(sid, subsample=n, crop_half=36.0)
        true_pose, _ = synth.make_pose(sid)
        return locref.transform_cloud_f32(true_pose, s)
    return [small_world["map"][::4], world_scan(3, 6000), world_scan(4, 5000)]


def origin_blob():
    """4 000 points across the world's origin, ±3 m: the voxels −2 … 2 of every axis, of which 0 is double width."""
    return (np.random.RandomState(12).rand(4000, 3) * 6.0 - 3.0).astype(np.float32)


def _clouds(locref, synth, small_world, method, extra):
    """The target's clouds: direct NDT sees `extra` as part of the map, incremental NDT as one more call."""
    if method == 2:
        return inc_clouds(locref, synth, small_world) + ([extra] if extra is not None else [])
    return [small_world["map"] if extra is None else np.vstack([small_world["map"], extra])]


def oracle_target(locref, synth, small_world, name, extra=None):
    """The oracle's matcher of case `name` with its target set."""
    method, nearby, th = CASES[name]
    ndt = locref.Ndt(method=method, nearby_type=nearby, res_outlier_th=th)
    for c in _clouds(locref, synth, small_world, method, extra):
        ndt.set_target(c)
    return ndt


def gpu_target(ctx, api, locref, synth, small_world, name, extra=None):
    """The same target on the context (an incremental voxel set is started afresh by the direct call in front of it)."""
    method, nearby, th = CASES[name]
    opts = api.ndt_opts(method=method, nearby_type=nearby, res_outlier_th=th)
    if method == 2:
        ctx.ndt_set_target(small_world["map"][:10], api.ndt_opts())
    for c in _clouds(locref, synth, small_world, method, extra):
        ctx.ndt_set_target(c, opts)


def restate(ndt, name, scan, pose):
    """ref.per_point of `scan` at `pose` against the oracle's dumped table."""
    method, nearby, th = CASES[name]
    keys, mu, info = ndt.dump()
    return ref.per_point(ref.Table(keys, mu, info), scan, pose, voxel_size=1.0, n_nearby=7 if nearby == 1 else 1, res_outlier_th=th,
                         weighted=method == 2)


def sample_points(small_world):
    """(512 points of scan10k spread over its rings, the pose they are evaluated at). The true pose: from init_pose, 0.3 m and 2° off,
    the gate refuses nine residuals in ten and four points in five would have nothing to compare."""
    return np.ascontiguousarray(small_world["scan10k"][::19][:512]), small_world["true_pose"]


def perturbed_poses(locref, pose, n=8):
    """n distinct poses a few cm and mrad from `pose` (the first is `pose` itself)."""
    rng = np.random.RandomState(77)
    out = [np.array(pose, dtype=np.float64)]
    for _ in range(n - 1):
        dx = np.concatenate([rng.uniform(-4e-3, 4e-3, 3), rng.uniform(-0.05, 0.05, 3)])
        out.append(locref.apply_update(pose, dx))
    return np.stack(out)


def accepted_pairs(name, H, eff):
    """The exact witness of the gate in one evaluation: the number of accepted (point, voxel) pairs. Direct NDT: H[3,3] = H[4,4] =
    H[5,5] (the identity block of JᵀJ, once per accepted pair, an integer held exactly in FP64); incremental NDT: effective_num."""
    if CASES[name][0] == 2:
        return int(eff)
    assert H[3, 3] == H[4, 4] == H[5, 5] and H[3, 3] == int(H[3, 3]), (H[3, 3], H[4, 4], H[5, 5])
    return int(H[3, 3])
