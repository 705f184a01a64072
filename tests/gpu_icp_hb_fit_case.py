"""Helper of tests/test_gpu_icp_hb.py::test_per_point_with_the_four_column_plane_fit: the P2Plane per-point rows (one-point scans
through icp_hb_batch) of the input sets in the .npz named first, written to the .npz named second. The library reads LOCGPU_PLANE_FIT
once per process, so the other plane fit is another process."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from loc_lib_amd import api  # noqa: E402
import icp_hb_cases as cases  # noqa: E402


def main(inp, out):
    d = np.load(inp)
    ctx = api.Context(0)
    res = {}
    for name in [k[5:] for k in d.files if k.startswith("scan_")]:
        ctx.icp_set_target(d["map_" + name])
        opts = api.icp_opts(method=api.P2PLANE, approximate=int(d["approximate_" + name]))
        res[name] = cases.one_point_rows(ctx, d["scan_" + name], d["pose_" + name], opts)
    ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
