#!/usr/bin/env python3
"""Randomised H, B, effective_num, ok parity probe (run ON the GPU box): the map kinds of fuzz_search.py, random scans and poses, all three ICP
methods (locgpu_icp_hb_batch) and direct and incremental NDT (locgpu_ndt_hb_batch; voxel size, nearby type, min_pts_in_voxel >= 3 and
res_outlier_th drawn the way fuzz_ndt.py draws them), GPU vs the oracle. Prints the worst relative error per map kind; returns 1 on any
effective_num / ok mismatch or on an H / B error above the project's bars (H 1e-9 of max|H|, B 1e-8 of max(|B|, 1e-6 max|H|)).

Two comparisons are ill-posed by construction of the input (deviations stated in INTEGRATION.md). Their effective_num and ok are held to
the oracle like everybody's; their H / B is held to a bar of its own, written here, and a breach counts in the return code:
  * point-to-plane ICP on the "lines" maps: every neighbourhood is five collinear points, the plane through them is not defined, and the
    null vector both sides pick by one rule amplifies the last bit of its inputs without bound. H and B must be finite and within
    ILL_RTOL = 1e-4 of the scales above: a decade over the largest figure of the recorded campaigns (1.5e-5, profiles/r04; 1.6e-7 since),
    five decades under an H or B that is plainly wrong.
  * direct NDT whose voxel TABLE differs from the oracle's: a voxel of exactly coplanar, collinear or coincident points (the "dups",
    "lines" and "lattice" maps make them) has singular values that are rounding noise, and the sign of such a value decides the sign of
    an eigenvalue of the information matrix (fuzz_ndt.py). The tables are compared first (same keys required). Where information
    matrices differ by more than 1e-7 the gate — the only place direct NDT uses them — accepts other pairs than the oracle's, so H and B
    are not the oracle's; they are held to what ANY set of accepted pairs gives: finite; H[3,3] = H[4,4] = H[5,5] = an integer number
    of pairs between 0 and nearby x points; every |H| entry <= pairs x max(1, |q|^2) and every |B| entry <= pairs x max(1, |q|) x reach,
    reach = the farthest a point can be from the mean of a voxel it probes (three voxel widths per axis: the cells touching 0 are
    double width).

    python tools/fuzz_hb.py [--cases 120] [--seed 11] [--max-log10-map 5.5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loc_lib_amd import api  # noqa: E402
from oracle import locref  # noqa: E402
import fuzz_search as fz  # noqa: E402

H_RTOL, B_RTOL = 1e-9, 1e-8
ILL_RTOL = 1e-4  # point-to-plane ICP on collinear maps (see above)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=120)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--max-log10-map", type=float, default=5.5, help="largest map, as log10 of its points (a short run caps it)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    kinds = ["uniform", "clusters", "sheets", "lines", "dups", "lattice"]
    worst = {k: 0.0 for k in kinds}
    effbad = singular = over = illposed = 0

    def compare(case, kind, label, hb, want, ill_posed=None):
        nonlocal effbad, singular, over, illposed
        ok, H, B, eff = want
        Hg, Bg, effg, okg = hb[:36].reshape(6, 6), hb[36:42], int(hb[42]), bool(hb[43])
        if eff != effg or ok != okg:
            # `ok` is `effective_num >= min && det(H) != 0` (icp_registration.cpp:204-211; ndt_registration.cpp:435-440). With equal
            # effective_num and an H that is singular to working precision (a handful of correspondences that all constrain the same
            # directions), whether the LU's last pivots come out as exact zeros is an accident of the summation order — in Eigen as much
            # as here: counted apart.
            sv = np.linalg.svd(H, compute_uv=False)
            if eff == effg and sv[-1] <= 1e-13 * sv[0]:
                singular += 1; print("ok differs on a numerically singular H (rank %d, effective_num %d):" % (int((sv > 1e-13 * sv[0]).sum()), eff), case, kind, label, ok, okg, flush=True)
            else:
                effbad += 1; print("EFF/OK differ", case, kind, label, eff, effg, ok, okg, flush=True)
        scale = max(np.abs(H).max(), 1e-300)
        scale_b = max(np.abs(B).max(), scale * 1e-6)
        eh, eb = np.abs(Hg - H).max() / scale, np.abs(Bg - B).max() / scale_b
        if ill_posed:
            illposed += 1
            good = ill_posed(Hg, Bg, eh, eb)
            print("ill-posed comparison, own bar %s:" % ("held" if good else "BROKEN"), case, kind, label, "H %.3e B %.3e" % (eh, eb), flush=True)
            if not good:
                over += 1
            return
        if not (eh <= H_RTOL and eb <= B_RTOL):  # a NaN on the GPU side fails too
            over += 1; print("H/B OVER THE BAR", case, kind, label, "H %.3e B %.3e" % (eh, eb), flush=True)
        worst[kind] = max(worst[kind], eh, eb * (H_RTOL / B_RTOL))

    def tables_differ(ctx, ref):
        """None when the device's direct-NDT table is the oracle's (same keys, information matrices within 1e-7), else what differs."""
        kg, _, ig = ctx.ndt_dump()
        ko, _, io = ref.dump()
        og, oo = np.lexsort(kg.T[::-1]), np.lexsort(ko.T[::-1])
        if kg.shape != ko.shape or not np.array_equal(kg[og], ko[oo]):
            return "KEYS"
        if len(kg) == 0:
            return None
        with np.errstate(invalid="ignore"):
            scale = np.abs(io[oo]).max(axis=(1, 2), keepdims=True) + 1e-300
            rel = (np.abs(ig[og] - io[oo]) / scale).max(axis=(1, 2))
        n = int((~(rel <= 1e-7) & ~(np.isnan(ig[og]).any(axis=(1, 2)) & np.isnan(io[oo]).any(axis=(1, 2)))).sum())
        return "%d of %d voxels with another information matrix" % (n, len(kg)) if n else None

    def collinear_plane_bar(Hg, Bg, eh, eb):
        return bool(np.isfinite(Hg).all() and np.isfinite(Bg).all() and eh <= ILL_RTOL and eb <= ILL_RTOL)

    def any_pairs_bar(scan, pose, voxel_size, n_nearby):
        """The bar of a direct-NDT evaluation against a table that is not the oracle's: what any set of accepted pairs gives."""
        q2 = float((scan.astype(np.float64) ** 2).sum(axis=1).max())
        reach = 3.0 * np.sqrt(3.0) * voxel_size

        def bar(Hg, Bg, eh, eb):
            if not (np.isfinite(Hg).all() and np.isfinite(Bg).all()):
                return False
            pairs = Hg[3, 3]
            if not (pairs == Hg[4, 4] == Hg[5, 5] and pairs == int(pairs) and 0 <= pairs <= n_nearby * len(scan)):
                return False
            return bool(np.abs(Hg).max() <= pairs * max(1.0, q2) * (1 + 1e-9) and np.abs(Bg).max() <= pairs * max(1.0, np.sqrt(q2)) * reach * (1 + 1e-9))
        return bar

    for case in range(a.cases):
        kind = kinds[case % 6]
        n = int(10 ** rng.uniform(2.0, min(5.5, a.max_log10_map)))
        cloud = fz.make_map(rng, kind, n).astype(np.float32)
        ctx = api.Context(0); ctx.icp_set_target(cloud)
        nq = int(10 ** rng.uniform(2.0, 4.3))
        scan = (cloud[rng.integers(0, len(cloud), nq)].astype(np.float64) + rng.normal(0, 10 ** rng.uniform(-3, -0.5), size=(nq, 3))).astype(np.float32)
        q = rng.normal(size=4) * np.array([0.02, 0.02, 0.02, 1.0]); q /= np.linalg.norm(q)
        pose = np.concatenate([q, rng.normal(0, 0.05, size=3)])
        b = ctx.batch([scan])
        for method in (api.P2PLANE, api.P2LINE, api.P2P):
            icp = locref.Icp(method=method); icp.set_target(cloud)
            compare(case, kind, "icp %d" % method, ctx.icp_hb_batch(b, pose[None], api.icp_opts(method=method))[0], icp.hb(scan, pose),
                    collinear_plane_bar if method == api.P2PLANE and kind == "lines" else None)
        for method in (api.DIRECT_NDT, api.INCREMENTAL_NDT):
            kw = dict(voxel_size=float(10 ** rng.uniform(-0.5, 0.5)), nearby_type=int(rng.integers(0, 2)), min_pts_in_voxel=int(rng.integers(3, 8)),
                      res_outlier_th=float(rng.choice([5.0, 20.0, 100.0])), min_effective_pts=int(rng.choice([10, 200])))
            ref = locref.Ndt(method=method, **kw)
            try:
                ctx.ndt_set_target(cloud, api.ndt_opts(method=method, **kw))
            except api.LocGpuError as e:  # a map beyond the ±2^20-voxel key range at this voxel size: nothing to compare
                print("ndt target refused", case, kind, kw, str(e)[:100], flush=True)
                continue
            ref.set_target(cloud)
            ill = tables_differ(ctx, ref) if method == api.DIRECT_NDT else None
            if ill == "KEYS":
                effbad += 1; print("NDT VOXEL KEYS differ", case, kind, kw, flush=True)
                continue
            if ill:
                print("direct NDT table differs:", ill, case, kind, flush=True)
            compare(case, kind, "ndt %d %s" % (method, kw), ctx.ndt_hb_batch(b, pose[None])[0], ref.hb(scan, pose),
                    any_pairs_bar(scan, pose, kw["voxel_size"], 7 if kw["nearby_type"] == 1 else 1) if ill else None)
        b.close()
        del ctx
    print("worst relative H/B error by map kind (B scaled to H's bar):", {k: float("%.2e" % v) for k, v in worst.items()}, "eff/ok mismatches:", effbad,
          "H/B over the bar:", over, "| ill-posed comparisons held to their own bars:", illposed,
          "| ok differs on a numerically singular H (not a mismatch: det == 0 there is a rounding accident on either side):", singular)
    return 1 if effbad or over else 0


if __name__ == "__main__":
    sys.exit(main())
