"""The CPU reference of the LOAM matcher's loop (loam_registration.cpp:38-99) as a composition of the oracle's pieces — what
tests/test_gpu_parity.py::test_cpp_facade_loam writes out inline: IcpRegistration::CaculateMatrixHAndB of the surface class (P2PLANE)
and of the edge class (P2LINE) at one pose, the sum of their normal equations, the 6×6 solve and the decoupled update."""
import numpy as np

LOAM_EPS = 1e-3        # LoamOption::eps_
LOAM_MAX_ITERATION = 20


def split_world(world):
    """The edge / surface split of the small world that test_cpp_facade_loam proves good on the oracle."""
    m, s = world["map"], world["scan10k"]
    return dict(edge_map=m[::5], surf_map=m, edge=s[::7], surf=s[np.arange(len(s)) % 7 != 0], init=np.array(world["init_pose"], dtype=np.float64))


class LoamOracle:
    def __init__(self, locref, edge_map, surf_map):
        self.locref = locref
        self.edge_icp = locref.Icp(method=locref.P2LINE)
        self.surf_icp = locref.Icp(method=locref.P2PLANE)
        self.edge_icp.set_target(edge_map)
        self.surf_icp.set_target(surf_map)

    def hb(self, edge, surf, pose):
        """(H, B, eff [surf, edge], ok [surf, edge]) of the sum; a class given as None adds nothing and reports 0 / True."""
        H, B, eff, ok = np.zeros((6, 6)), np.zeros(6), [0, 0], [True, True]
        for c, (icp, src) in enumerate(((self.surf_icp, surf), (self.edge_icp, edge))):
            if src is None:
                continue
            ok[c], Hc, Bc, eff[c] = icp.hb(src, pose)
            H, B = H + Hc, B + Bc
        return H, B, eff, ok

    def scan_match(self, edge, surf, init, eps=LOAM_EPS, max_iteration=LOAM_MAX_ITERATION):
        """dict(pose, iterations, status, converged): converged = the loop left through |dx| < eps; status 0, or 3 / 4 when the surface / edge evaluation reported false (surface first); the
        pose of a failed alignment is the initial one (the reference returns before it writes result_pose)."""
        p = np.array(init, dtype=np.float64)
        iterations, converged = 0, False
        for _ in range(max_iteration):
            H, B, _, ok = self.hb(edge, surf, p)
            iterations += 1
            if not ok[0] or not ok[1]:
                return dict(pose=np.array(init, dtype=np.float64), iterations=iterations, status=3 if not ok[0] else 4, converged=False)
            det, dx = self.locref.lu6(H, B)
            if det == 0.0:  # the reference would divide by zero; the library makes no update and goes on
                continue
            p = self.locref.apply_update(p, dx)
            if np.linalg.norm(dx) < eps:
                converged = True
                break
        return dict(pose=p, iterations=iterations, status=0, converged=converged)
