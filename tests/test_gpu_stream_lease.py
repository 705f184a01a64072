"""A compute stream is leased per alignment (csrc/stream_lease.hpp; align_begin / align_finish in csrc/gn_driver.hip): a caller that
rotates more batches than the context has streams — bench.py's four batches with three alignments in flight — still has every alignment
in flight on a stream of its own, a batch that moves keeps the order with its upload, and nothing moves a bit of any result: every
alignment here is compared bitwise with a blocking align_batch of the same scans in a batch of the same shape.

Small shapes: six scans of 2-3.3 k points against the 200 k-point local map, P2Plane ICP and direct NDT."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SCANS, N_SETS, N_BATCHES, DEPTH, STEPS = 6, 8, 4, 3, 12


@pytest.fixture(scope="module")
def world(api, small_world):
    """A context of its own (its first four batches are dealt streams 0, 1, 2, 0) with both targets; eight different scans, dealt
    to N_SETS sets of six; and the blocking reference of every (method, set), made once."""
    s = small_world["scan10k"]
    pool = [np.ascontiguousarray(s[i::3]) for i in range(3)] + [np.ascontiguousarray(s[i::4]) for i in range(4)] + [small_world["scan2k"]]
    sets = [[pool[(g + j) % len(pool)] for j in range(N_SCANS)] for g in range(N_SETS)]
    max_points = max(len(p) for p in pool)
    inits = np.tile(np.asarray(small_world["init_pose"], np.float64), (N_SCANS, 1))
    inits[:, 4:] += 0.01 * np.arange(N_SCANS)[:, None] * np.array([1.0, -1.0, 0.5])  # no two scans of a batch start alike
    ctx = api.Context(0)
    ctx.icp_set_target(small_world["map"])
    ctx.ndt_set_target(small_world["map"])
    w = dict(ctx=ctx, sets=sets, max_points=max_points, inits=inits, opts=api.icp_opts(method=api.P2PLANE), ref={})
    rb = ctx.batch_empty(N_SCANS, max_points)
    for method in ("p2plane", "ndt"):
        for g in range(N_SETS):
            rb.upload_async(sets[g])
            w["ref"][method, g] = ctx.ndt_align_batch(rb, inits) if method == "ndt" else ctx.icp_align_batch(rb, inits, w["opts"])
    rb.close()
    yield w
    ctx.close()


def _begin(w, method, b):
    if method == "ndt":
        w["ctx"].ndt_align_batch_begin(b, w["inits"])
    else:
        w["ctx"].icp_align_batch_begin(b, w["inits"], w["opts"])


def _same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1] == want[1]


def _batches(w, n=N_BATCHES):
    return [w["ctx"].batch_empty(N_SCANS, w["max_points"]) for _ in range(n)]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("method", ["p2plane", "ndt"])
def test_bench_rotation_keeps_the_alignments_in_flight_on_different_streams(world, method, graph):
    """bench.py's streaming loop: begin step g on batch g % 4, start the copy of step g + 1's scans into the next batch, at most three
    in flight, ended in order. At every end the batches in flight hold pairwise different streams, and every step returns what a
    blocking align_batch of its scans returns, bit for bit — eager and under graph replay."""
    ctx = world["ctx"]
    bufs = _batches(world)
    try:
        ctx.graph_enable(graph)
        assert [b.debug_slot() for b in bufs] in ([0, 1, 2, 0], [1, 2, 0, 1], [2, 0, 1, 2])  # dealt in turn: two of four share a stream
        bufs[0].upload_async(world["sets"][0])
        inflight, begun, ended = [], 0, 0
        while begun < STEPS or inflight:
            while begun < STEPS and len(inflight) < DEPTH:
                b = bufs[begun % N_BATCHES]
                _begin(world, method, b)
                bufs[(begun + 1) % N_BATCHES].upload_async(world["sets"][(begun + 1) % N_SETS])
                inflight.append((begun, b))
                begun += 1
            slots = [b.debug_slot() for _, b in inflight]
            assert all(0 <= s < 3 for s in slots) and len(set(slots)) == len(slots), (ended, slots)
            g, b = inflight.pop(0)
            got = ctx.align_batch_end(b)
            assert _same(got, world["ref"][method, g % N_SETS]), (method, graph, g)
            ended += 1
        assert ended == STEPS
    finally:
        ctx.graph_enable(False)
        for b in bufs:
            b.upload_wait()
            b.close()


@pytest.mark.parametrize("method", ["p2plane", "ndt"])
def test_more_alignments_in_flight_than_streams(world, method):
    """Four in flight on three streams: loads {2, 1, 1}. The youngest — queued behind its stream-mate — can be ended first; the next
    begin takes the stream that came free; every result is the blocking call's."""
    ctx = world["ctx"]
    bufs = _batches(world)
    try:
        for i, b in enumerate(bufs):
            b.upload_async(world["sets"][i])
        for b in bufs:
            _begin(world, method, b)
        slots = [b.debug_slot() for b in bufs]
        assert sorted(np.bincount(slots, minlength=3).tolist()) == [1, 1, 2], slots
        mate = [i for i in range(3) if slots[i] == slots[3]]
        assert len(mate) == 1  # the fourth went to the lowest of three equally loaded streams, beside ONE other batch
        assert _same(ctx.align_batch_end(bufs[3]), world["ref"][method, 3])
        # a stream comes free: the batch whose own stream is still taken goes there
        free = next(i for i in range(3) if i != mate[0])
        assert _same(ctx.align_batch_end(bufs[free]), world["ref"][method, free])
        bufs[3].upload_async(world["sets"][5])
        _begin(world, method, bufs[3])
        assert bufs[3].debug_slot() == slots[free] != slots[mate[0]]
        live = [b.debug_slot() for i, b in enumerate(bufs) if i != free]
        assert len(set(live)) == 3, live
        assert _same(ctx.align_batch_end(bufs[3]), world["ref"][method, 5])
        for i in range(3):
            if i != free:
                assert _same(ctx.align_batch_end(bufs[i]), world["ref"][method, i])
        # everything ended: a batch begun now stays where it is
        before = bufs[3].debug_slot()
        _begin(world, method, bufs[3])
        assert bufs[3].debug_slot() == before
        assert _same(ctx.align_batch_end(bufs[3]), world["ref"][method, 5])
    finally:
        for b in bufs:
            b.upload_wait()
            b.close()


@pytest.mark.parametrize("graph", [False, True])
def test_a_batch_that_moves_keeps_the_order_with_its_upload_and_with_later_calls(world, graph):
    """A batch whose stream is taken moves at its begin: the alignment reads the scans of the upload started before that begin, not
    the ones the batch held; a locgpu_batch_preprocess on it afterwards gives what it gives on a batch that never moved."""
    ctx = world["ctx"]
    bufs = _batches(world)
    never, dst_a, dst_b = _batches(world, 3)
    try:
        ctx.graph_enable(graph)
        a, moved = bufs[0], bufs[3]
        assert a.debug_slot() == moved.debug_slot()
        a.upload_async(world["sets"][1])
        moved.upload_async(world["sets"][2])
        assert _same(ctx.icp_align_batch(moved, world["inits"], world["opts"]), world["ref"]["p2plane", 2])  # used once on its own stream
        home = moved.debug_slot()
        _begin(world, "p2plane", a)
        moved.upload_async(world["sets"][6])  # other scans, on their way when the alignment begins
        _begin(world, "p2plane", moved)
        assert moved.debug_slot() != home and moved.debug_slot() != a.debug_slot()
        got = ctx.align_batch_end(moved)
        assert _same(got, world["ref"]["p2plane", 6]) and not _same(got, world["ref"]["p2plane", 2])
        assert _same(ctx.align_batch_end(a), world["ref"]["p2plane", 1])
        never.upload_async(world["sets"][6])
        cm, sm = moved.preprocess(0.5, out=dst_a)
        cn, sn = never.preprocess(0.5, out=dst_b)
        assert np.array_equal(cm, cn) and np.array_equal(sm, sn) and cm.min() > 0
        for s in range(N_SCANS):
            assert dst_a.download_scan(s).tobytes() == dst_b.download_scan(s).tobytes(), s
        # and the moved batch aligns as before from where it now is
        assert _same(ctx.icp_align_batch(moved, world["inits"], world["opts"]), world["ref"]["p2plane", 6])
    finally:
        ctx.graph_enable(False)
        for b in bufs + [never, dst_a, dst_b]:
            b.upload_wait()
            b.close()


def test_a_one_scan_batch_that_moves_leaves_its_paced_tail_behind(world):
    """A blocking one-scan alignment is paced from the host and may leave a few idle launches queued on its stream. When the batch moves
    at its next begin, the new stream is ordered behind them: the alignment on the new stream gives the blocking call's bits, again
    and again, while its old stream carries another batch's alignment."""
    ctx = world["ctx"]
    scan_a, scan_b = world["sets"][0][0], world["sets"][0][1]
    init = world["inits"][:1]
    ones = [ctx.batch_empty(1, world["max_points"]) for _ in range(N_BATCHES)]
    big = ones[0]
    try:
        mover = ones[3]
        assert mover.debug_slot() == big.debug_slot()
        mover.upload_async([scan_a])
        want_a = ctx.icp_align_batch(mover, init, world["opts"])  # paced, on the stream it was dealt
        home = mover.debug_slot()
        mover.upload_async([scan_b])
        want_b = ctx.icp_align_batch(mover, init, world["opts"])
        assert mover.debug_slot() == home and not _same(want_a, want_b)
        big.upload_async([scan_a])
        for rep in range(3):
            ctx.icp_align_batch_begin(big, init, world["opts"])
            mover.upload_async([scan_a if rep % 2 == 0 else scan_b])
            got = ctx.icp_align_batch(mover, init, world["opts"])  # its stream is taken: moves (first round), paced again
            assert mover.debug_slot() != big.debug_slot()
            assert _same(got, want_a if rep % 2 == 0 else want_b), rep
            assert _same(ctx.align_batch_end(big), want_a), rep
    finally:
        for b in ones:
            b.upload_wait()
            b.close()
