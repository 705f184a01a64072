"""The numpy restatement of the range-image ingest (tests/range_image_ref.py) against cells computed by hand: the definition in
include/locgpu.h, one float32 operation per step, CloudConver::Conver's two rules (cloud_subscriber.cpp:7-29,
point_cloud_utils.h:41-44)."""
from types import SimpleNamespace

import numpy as np

import range_image_ref as ref

F = np.float32


def _model(n_rings, n_cols, range_scale, min_range, cos_el, sin_el, cos_az, sin_az):
    return SimpleNamespace(n_rings=n_rings, n_cols=n_cols, range_scale=F(range_scale), min_range=F(min_range), cos_el=np.asarray(cos_el, F),
                           sin_el=np.asarray(sin_el, F), cos_az=np.asarray(cos_az, F), sin_az=np.asarray(sin_az, F))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_hand_computed_cells_and_ring_major_order():
    # binary fractions throughout: every product below is exact, so the expected values need no rounding argument
    m = _model(2, 3, 0.25, 0.0, [1.0, 0.5], [0.0, 0.75], [1.0, 0.0, -0.5], [0.0, 1.0, 0.5])
    image = np.array([[4, 0, 8], [0, 16, 2]], np.uint16)
    pts, rings = ref.decode(m, image)
    # ring 0: r = 1 → (1, 0, 0); count 0 dropped; r = 2 → (−1, 1, 0). ring 1: r = 4, h = 2 → (0, 2, 3); r = 0.5, h = 0.25 → (−0.125, 0.125, 0.375)
    want = np.array([[1, 0, 0, 0], [-1, 1, 0, 0], [0, 2, 3, 0], [-0.125, 0.125, 0.375, 0]], F)
    assert pts.dtype == F and rings.dtype == np.uint8
    assert np.array_equal(pts, want) and not _bits(pts[:, 3]).any()
    assert rings.tolist() == [0, 0, 1, 1]  # ring-major, columns ascending inside a ring
    # per-laser azimuth tables: a = g * n_cols + c
    m2 = _model(2, 3, 0.25, 0.0, [1.0, 0.5], [0.0, 0.75], [[1.0, 0.0, -0.5], [0.5, 1.0, 0.0]], [[0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
    pts2, rings2 = ref.decode(m2, image)
    want2 = np.array([[1, 0, 0, 0], [-1, 1, 0, 0], [2, 0, 3, 0], [0, 0.25, 0.375, 0]], F)
    assert np.array_equal(pts2, want2) and rings2.tolist() == [0, 0, 1, 1]


def test_a_count_of_zero_is_dropped_and_min_range_zero_keeps_all():
    m = _model(1, 4, 1.0, 0.0, [1.0], [0.0], [1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])
    pts, rings = ref.decode(m, np.array([0, 1, 1, 0], np.uint16))
    # cell 2 decodes to (0, 0, 0): distance 0 is not < 0, so min_range = 0 keeps it; the two zero counts yield nothing
    assert np.array_equal(pts, np.array([[1, 0, 0, 0], [0, 0, 0, 0]], F)) and rings.tolist() == [0, 0]
    every = ref.decode(m, np.array([7, 1, 65535, 3], np.uint16))[0]
    assert len(every) == 4 and every[2, 0] == 0 and every[0, 0] == 7


def test_the_cut_is_sqrtf_less_than_min_range():
    """min_range = 5. Cell 0: (3, 4, 0), distance exactly 5 — kept. Cell 1: (prev(5), 0, 0), the next float32 below — dropped.
    Cell 2: (3, 4 − 2^-22, 0): y·y = 16 − 2^-19 (+ 2^-44, rounded away), the sum is 25 − 2^-19, the float32 just below 25, and its
    square root 5 − 1.9e-7 rounds to 5.0 (the spacing below 5 is 4.8e-7) — kept by sqrtf(...) < min_range, where a squared shortcut
    (sum < 25) would drop it."""
    below5 = np.nextafter(F(5), F(0))
    y = np.nextafter(F(4), F(0))
    assert float(y) == 4.0 - 2.0 ** -22
    m = _model(1, 3, 1.0, 5.0, [1.0], [0.0], [3.0, below5, 3.0], [4.0, 0.0, y])
    pts, rings = ref.decode(m, np.array([1, 1, 1], np.uint16))
    s = F(3) * F(3) + y * y
    assert s == np.nextafter(F(25), F(0)) and s < F(25) and np.sqrt(s) == F(5)
    assert np.array_equal(_bits(pts[:, :3]), _bits(np.array([[3, 4, 0], [3, y, 0]], F)))
    assert rings.tolist() == [0, 0]
    # the same cells with the reference's 4.0 and a cut nothing reaches
    assert len(ref.decode(_model(1, 3, 1.0, 4.0, [1.0], [0.0], [3.0, below5, 3.0], [4.0, 0.0, y]), np.ones(3, np.uint16))[0]) == 3
    assert len(ref.decode(_model(1, 3, 1.0, 5.5, [1.0], [0.0], [3.0, below5, 3.0], [4.0, 0.0, y]), np.ones(3, np.uint16))[0]) == 0


def test_a_non_finite_table_entry_drops_its_cells():
    m = _model(2, 3, 1.0, 0.0, [1.0, np.inf], [0.0, 0.0], [1.0, np.nan, 1.0], [0.0, 0.0, 0.0])
    pts, rings = ref.decode(m, np.full((2, 3), 9, np.uint16))
    # ring 1 (cos_el = inf → x = inf, y = inf · 0 = NaN) and column 1 (NaN) are gone
    assert np.array_equal(pts, np.array([[9, 0, 0, 0], [9, 0, 0, 0]], F)) and rings.tolist() == [0, 0]
    # an overflowing product drops the cell too: 65535 · 3e38 = inf
    big = _model(1, 2, 3e38, 0.0, [1.0], [0.0], [1.0, 1.0], [0.0, 0.0])
    pts, _ = ref.decode(big, np.array([1, 65535], np.uint16))
    assert len(pts) == 1 and pts[0, 0] == F(3e38)
