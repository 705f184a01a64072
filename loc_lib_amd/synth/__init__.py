"""Synthetic world ``cityblock-v1``: ctypes binding of ``cityblock.cpp``.

Deterministic map / scan / pose generator shared by the tests, ``bench.py`` and the CPU baseline.
Host-only utility; not part of the registration hot path.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libcityblock.so")

WORLD_SEED = 20240901
SCAN_SEED_BASE = 777
PERTURB_SEED = 4242
MAP_SIGMA = 0.01
RANGE_SIGMA = 0.02
N_BEAMS = 64
N_AZ = 1800


def build(force=False):
    """Compile libcityblock.so in-tree (g++)."""
    src = os.path.join(_HERE, "cityblock.cpp")
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-o", _LIB_PATH, src])
    return _LIB_PATH


_lib = None


def _load():
    global _lib
    if _lib is None:
        build()
        lib = ctypes.CDLL(_LIB_PATH)
        lib.cityblock_map.argtypes = [ctypes.c_uint64, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t]
        lib.cityblock_map.restype = None
        lib.cityblock_scan.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t]
        lib.cityblock_scan.restype = ctypes.c_size_t
        lib.cityblock_pose.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                       ctypes.c_void_p]
        lib.cityblock_pose.restype = None
        lib.cityblock_map_local.argtypes = [ctypes.c_uint64, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t]
        lib.cityblock_map_local.restype = None
        lib.cityblock_sensor.argtypes = [ctypes.c_int, ctypes.c_void_p]
        lib.cityblock_sensor.restype = None
        _lib = lib
    return _lib


def make_map(n, seed=WORLD_SEED, sigma=MAP_SIGMA, stride=3):
    """n map points, float32 [n, stride] (xyz in the first three columns, rest zero)."""
    out = np.zeros((n, stride), dtype=np.float32)
    _load().cityblock_map(seed, n, sigma, out.ctypes.data, stride)
    return out


def sensor_position(scan_id):
    """(x, y, z, yaw) of the sensor for ``scan_id``."""
    out = np.zeros(4)
    _load().cityblock_sensor(scan_id, out.ctypes.data)
    return out


def make_local_map(n, scan_id, half=30.0, seed=WORLD_SEED, sigma=MAP_SIGMA, stride=3):
    """n map points inside the ±half square around scan ``scan_id``'s sensor (a box-cropped local map)."""
    c = sensor_position(scan_id)
    out = np.zeros((n, stride), dtype=np.float32)
    _load().cityblock_map_local(seed, n, sigma, c[0], c[1], half, out.ctypes.data, stride)
    return out


def make_scan(scan_id, n_beams=N_BEAMS, n_az=N_AZ, world_seed=WORLD_SEED, range_sigma=RANGE_SIGMA, stride=3, subsample=None,
              crop_half=None):
    """Scan ``scan_id`` of the circuit in the sensor frame, float32 [m, stride], ring-major.

    ``crop_half``: keep only returns whose true world position lies within ±crop_half (x, y) of the sensor — pairs a scan
    with ``make_local_map(half > crop_half)`` the way the reference's ±150 m local map always contains its scans.
    """
    out = np.zeros((n_beams * n_az, stride), dtype=np.float32)
    m = _load().cityblock_scan(world_seed, scan_id, SCAN_SEED_BASE + scan_id, n_beams, n_az, range_sigma, out.ctypes.data, stride)
    out = out[:m]
    if crop_half is not None:
        yaw = sensor_position(scan_id)[3]
        c, s_ = np.cos(yaw), np.sin(yaw)
        wx = c * out[:, 0] - s_ * out[:, 1]
        wy = s_ * out[:, 0] + c * out[:, 1]
        out = np.ascontiguousarray(out[(np.abs(wx) <= crop_half) & (np.abs(wy) <= crop_half)])
        m = len(out)
    if subsample is not None and subsample < m:
        idx = np.floor(np.arange(subsample) * (m / subsample)).astype(np.int64)
        out = np.ascontiguousarray(out[idx])
    return out


def make_pose(scan_id, trans_amp=0.3, rot_amp_deg=2.0, seed=PERTURB_SEED):
    """(true_pose7, init_pose7): quaternion xyzw + translation (Sophus::SE3d::data() order)."""
    t = np.zeros(7)
    i = np.zeros(7)
    _load().cityblock_pose(scan_id, seed, trans_amp, np.deg2rad(rot_amp_deg), t.ctypes.data, i.ctypes.data)
    return t, i


def sensor_tables(n_rings=N_BEAMS, n_cols=N_AZ):
    """(cos_el, sin_el, cos_az, sin_az) of the generator's beams as float32 tables: ring g at +2.0 … −24.8 deg, column c at 2π c / n_cols —
    what a range-image sensor model of this LiDAR is made of."""
    g = np.arange(n_rings, dtype=np.float64)
    el = np.deg2rad(2.0 - (26.8 * g / (n_rings - 1) if n_rings > 1 else 0.0 * g))
    az = 2.0 * np.pi * np.arange(n_cols, dtype=np.float64) / n_cols
    return tuple(t.astype(np.float32) for t in (np.cos(el), np.sin(el), np.cos(az), np.sin(az)))


def make_range_image(scan_id, model, **scan_args):
    """Scan ``scan_id`` as the range image a spinning LiDAR delivers: uint16 [n_rings, n_cols], 0 = no return. Test and tool
    infrastructure, numpy only: the points of ``make_scan(scan_id, n_beams=n_rings, n_az=n_cols)`` are binned into the model's cells by
    elevation (nearest ring of the model's tables) and azimuth (nearest column), and the range is quantised with ``range_scale``
    (counts clipped to 1..65535; of two returns in one cell the later one stays). ``model`` needs n_rings, n_cols, range_scale and the
    four tables (api.SensorModel, or anything shaped like it)."""
    n_rings, n_cols = int(model.n_rings), int(model.n_cols)
    pts = make_scan(scan_id, n_beams=n_rings, n_az=n_cols, **scan_args)[:, :3].astype(np.float64)
    image = np.zeros((n_rings, n_cols), np.uint16)
    if len(pts) == 0:
        return image
    rng = np.sqrt((pts * pts).sum(1))
    el = np.arcsin(np.clip(pts[:, 2] / np.maximum(rng, 1e-12), -1.0, 1.0))
    az = np.arctan2(pts[:, 1], pts[:, 0])
    ring_el = np.arctan2(np.asarray(model.sin_el, np.float64), np.asarray(model.cos_el, np.float64))
    order = np.argsort(ring_el, kind="stable")
    hi = np.clip(np.searchsorted(ring_el[order], el), 1, n_rings - 1) if n_rings > 1 else np.zeros(len(el), np.int64)
    lo = np.maximum(hi - 1, 0)
    ring = order[np.where(np.abs(el - ring_el[order][lo]) <= np.abs(el - ring_el[order][hi]), lo, hi)]
    cos_az, sin_az = np.asarray(model.cos_az, np.float64), np.asarray(model.sin_az, np.float64)
    az0 = np.arctan2(sin_az.reshape(-1, n_cols)[:, 0], cos_az.reshape(-1, n_cols)[:, 0])  # per ring with per-laser offsets, else one entry
    az0 = az0[ring] if len(az0) == n_rings and cos_az.ndim == 2 else az0[0]
    col = np.rint((az - az0) / (2.0 * np.pi) * n_cols).astype(np.int64) % n_cols
    image[ring, col] = np.clip(np.rint(rng / float(model.range_scale)), 1, 65535).astype(np.uint16)
    return image
