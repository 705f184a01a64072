"""The run flags of the search stage (csrc/icp_search.hip, SearchArgs::run_flags) restated in numpy, for tests/test_gpu_run_flags.py
and tests/test_run_flags_ref.py. A scan's points are taken in groups of 64 (the walk kernel's waves); a point is a LEADER of the plane
fit when its neighbour set is not known to be the set of the point before it, a FOLLOWER otherwise."""
import numpy as np


def unpack_flags(words, n):
    """words: uint64 [ceil(n / 64)] (or more) → bool [n], True = leader: bit j of word w belongs to point 64 w + j."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint64)[:(n + 63) // 64])
    bits = np.unpackbits(w.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
    return bits[:n].astype(bool)


def leaders(nn, unknown=None):
    """nn: int [n, 5] neighbour indices of consecutive points, -1 = none. unknown (optional): bool [n], the points whose list the
    deciding kernel cannot see. → bool [n]: the point is lane 0 of its group of 64, or has no full list, or is unknown, or follows
    an unknown point, or its SET of five differs from the previous point's (the order within a list does not count)."""
    nn = np.asarray(nn)
    n = len(nn)
    srt = np.sort(nn, axis=1)
    lead = (np.arange(n) % 64) == 0
    lead |= (nn < 0).any(axis=1)
    differs = np.ones(n, dtype=bool)
    differs[1:] = (srt[1:] != srt[:-1]).any(axis=1)
    lead |= differs
    if unknown is not None:
        unknown = np.asarray(unknown, dtype=bool)
        lead |= unknown
        lead[1:] |= unknown[:-1]
    return lead
