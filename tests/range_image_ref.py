"""Range-image ingest restated in numpy float32 (include/locgpu.h, "Range-image ingest"): the decode of a cell and
CloudConver::Conver's two rules (LocUtils/src/subscriber/cloud_subscriber.cpp:7-29, common/point_cloud_utils.h:41-44), each operation
one float32 operation rounded to nearest, nothing fused. Test infrastructure: what locgpu_batch_upload_ranges and
locgpu_cloud_upload_ranges are held to byte for byte.

A model is anything with n_rings, n_cols, range_scale, min_range and the tables cos_el, sin_el [n_rings], cos_az, sin_az
[n_cols] or [n_rings, n_cols] (api.SensorModel is one)."""
import numpy as np

F = np.float32


def decode(model, image):
    """(points [n, 4] float32 {x, y, z, +0}, rings [n] uint8) of one image, survivors in ring-ascending, then column-ascending order."""
    n_rings, n_cols = int(model.n_rings), int(model.n_cols)
    k = np.ascontiguousarray(image, dtype=np.uint16).reshape(n_rings, n_cols)
    cos_el, sin_el = (np.asarray(t, F).reshape(n_rings, 1) for t in (model.cos_el, model.sin_el))
    cos_az, sin_az = (np.asarray(t, F) for t in (model.cos_az, model.sin_az))
    if cos_az.ndim == 1:  # a = c
        cos_az, sin_az = cos_az.reshape(1, n_cols), sin_az.reshape(1, n_cols)
    else:                 # a = g * n_cols + c
        cos_az, sin_az = cos_az.reshape(n_rings, n_cols), sin_az.reshape(n_rings, n_cols)
    with np.errstate(all="ignore"):
        r = k.astype(F) * F(model.range_scale)
        h = r * cos_el
        x = h * cos_az
        y = h * sin_az
        z = r * sin_el
        assert r.dtype == h.dtype == x.dtype == y.dtype == z.dtype == F
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        d = np.sqrt((x * x + y * y) + z * z)  # PointDistance: products and sums each rounded to float32
        assert d.dtype == F
        keep = (k != 0) & finite & ~(d < F(model.min_range))
    g, c = np.nonzero(keep)  # row-major: ring-ascending, then column-ascending
    pts = np.zeros((len(g), 4), F)
    pts[:, 0], pts[:, 1], pts[:, 2] = x[g, c], y[g, c], z[g, c]
    return pts, g.astype(np.uint8)
