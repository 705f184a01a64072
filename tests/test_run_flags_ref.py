"""tests/run_flags_ref.py — the numpy restatement of the search stage's run flags that tests/test_gpu_run_flags.py measures the kernel
against — on hand-made lists (no GPU)."""
import numpy as np

from run_flags_ref import leaders, unpack_flags


def test_equal_sets_in_another_order_follow():
    nn = np.array([[1, 2, 3, 4, 5], [5, 4, 3, 2, 1], [2, 1, 3, 5, 4], [1, 2, 3, 4, 5]])
    assert leaders(nn).tolist() == [True, False, False, False]


def test_a_differing_fifth_neighbour_leads():
    nn = np.array([[1, 2, 3, 4, 5], [1, 2, 3, 4, 6], [1, 2, 3, 4, 6], [6, 1, 2, 3, 4], [1, 2, 3, 4, 5]])
    assert leaders(nn).tolist() == [True, True, False, False, True]


def test_lane_zero_of_every_group_of_64_leads():
    nn = np.tile(np.array([[7, 8, 9, 10, 11]]), (130, 1))
    want = np.zeros(130, dtype=bool)
    want[[0, 64, 128]] = True
    assert np.array_equal(leaders(nn), want)


def test_a_point_without_a_full_list_leads_and_so_does_the_point_behind_it():
    nn = np.array([[1, 2, 3, 4, 5], [-1, -1, -1, -1, -1], [-1, -1, -1, -1, -1], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [1, 2, 3, 4, -1], [1, 2, 3, 4, -1]])
    assert leaders(nn).tolist() == [True, True, True, True, False, True, True]


def test_neighbouring_unknown_points_are_never_equal():
    """Two unknown points in a row hold whatever the kernel left in their registers — here equal lists: both lead, and so does the
    known point behind them, whatever its list."""
    nn = np.tile(np.array([[1, 2, 3, 4, 5]]), (6, 1))
    unknown = np.array([False, False, True, True, False, False])
    assert leaders(nn, unknown).tolist() == [True, False, True, True, True, False]
    assert leaders(nn).tolist() == [True, False, False, False, False, False]


def test_unpack_flags_takes_bit_j_of_word_w_for_point_64w_plus_j():
    words = np.array([(1 << 0) | (1 << 5) | (1 << 63), 1 | (1 << 1)], dtype=np.uint64)
    bits = unpack_flags(words, 70)
    assert bits.shape == (70,) and np.flatnonzero(bits).tolist() == [0, 5, 63, 64, 65]
