// loc_lib_amd/csrc/stream_lease.hpp — which of a context's compute streams an alignment runs on (gn_driver.hip: align_begin takes the
// lease, align_finish gives it back). Plain C++ with no HIP in it, so that the CPU suite checks the rule (tests/cpp/stream_lease_check.cpp).
//
// A batch used to keep the stream it was dealt at creation. A streaming caller with three alignments in flight rotates FOUR batches
// (the copy for the next step must not land in a batch an alignment reads), so two of them shared one of the three streams and were
// in flight together in two steps of every four: the later one's first chunk queued behind the earlier one's, and the earlier one's
// further chunks behind that (profiles/stream_lease.md). The stream is therefore leased per ALIGNMENT: an alignment keeps its batch's
// stream while no other alignment in flight is on it, and otherwise goes to the least-loaded one.
#pragma once

namespace locgpu {

// load[i]: alignments begun and not ended on stream i of n, the one being begun NOT among them; `current`: the stream the batch
// holds. Returns `current` when nobody else is on it — a caller with no more batches than streams never moves — and otherwise a
// stream of minimal load, the lowest index on ties (which may be `current` again: moving would gain nothing). Always in [0, n).
inline int lease_choose(const int* load, int n, int current) {
    if (current >= 0 && current < n && load[current] == 0) return current;
    int best = 0;
    for (int i = 1; i < n; ++i)
        if (load[i] < load[best]) best = i;
    return best;
}

}  // namespace locgpu
