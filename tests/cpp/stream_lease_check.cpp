// tests/cpp/stream_lease_check.cpp — the rule that picks an alignment's compute stream (loc_lib_amd/csrc/stream_lease.hpp) on the CPU:
// exhaustive over loads 0..3 on three streams and every current stream, against the rule as the header words it. Then the
// streaming rotation the rule is there for (four batches, three alignments in flight, FIFO end) as bookkeeping only: after the
// pipeline has filled, the alignments in flight sit on pairwise different streams at every end.
#include <cstdio>
#include <vector>

#include "stream_lease.hpp"

using locgpu::lease_choose;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            failures++;                                   \
        }                                                 \
    } while (0)

static void exhaustive() {
    constexpr int n = 3;
    int cases = 0;
    for (int a = 0; a <= 3; ++a)
        for (int b = 0; b <= 3; ++b)
            for (int c = 0; c <= 3; ++c)
                for (int cur = 0; cur < n; ++cur) {
                    const int load[n] = {a, b, c};
                    const int got = lease_choose(load, n, cur);
                    cases++;
                    CHECK(got >= 0 && got < n, "loads %d %d %d, current %d: %d is no stream", a, b, c, cur, got);
                    if (got < 0 || got >= n) continue;
                    if (load[cur] == 0) {  // nobody else on it: stay
                        CHECK(got == cur, "loads %d %d %d: left the free current stream %d for %d", a, b, c, cur, got);
                        continue;
                    }
                    // somebody else holds it: a stream of minimal load, the lowest index among those
                    int want = 0;
                    for (int i = 1; i < n; ++i)
                        if (load[i] < load[want]) want = i;
                    CHECK(got == want, "loads %d %d %d, current %d: got %d, the least loaded is %d", a, b, c, cur, got, want);
                    // it stays on a stream somebody else holds only when no other stream is lighter
                    if (got == cur)
                        for (int i = 0; i < n; ++i) CHECK(load[i] >= load[cur], "loads %d %d %d: stayed on %d though %d is lighter", a, b, c, cur, i);
                }
    // a stream index from nowhere never comes back out
    const int load[n] = {1, 0, 2};
    for (int cur : {-1, 3, 1000}) CHECK(lease_choose(load, n, cur) == 1, "current %d out of range", cur);
    printf("exhaustive: %d cases OK\n", cases);
}

static void rotation(int n_batches, int depth, int steps) {
    constexpr int n = 3;
    int load[n] = {0, 0, 0};
    std::vector<int> slot((size_t)n_batches);
    for (int i = 0; i < n_batches; ++i) slot[(size_t)i] = i % n;  // dealt in turn at creation
    std::vector<int> inflight;
    int begun = 0, moves = 0;
    while (begun < steps || !inflight.empty()) {
        while (begun < steps && (int)inflight.size() < depth) {
            const int b = begun++ % n_batches;
            const int to = lease_choose(load, n, slot[(size_t)b]);
            moves += to != slot[(size_t)b];
            slot[(size_t)b] = to;
            load[to]++;
            inflight.push_back(b);
        }
        if ((int)inflight.size() <= n)
            for (size_t i = 0; i < inflight.size(); ++i)
                for (size_t j = i + 1; j < inflight.size(); ++j)
                    CHECK(slot[(size_t)inflight[i]] != slot[(size_t)inflight[j]], "%d batches, depth %d: batches %d and %d in flight on stream %d", n_batches, depth,
                          inflight[i], inflight[j], slot[(size_t)inflight[i]]);
        load[slot[(size_t)inflight.front()]]--;
        inflight.erase(inflight.begin());
    }
    for (int i = 0; i < n; ++i) CHECK(load[i] == 0, "stream %d keeps load %d", i, load[i]);
    if (n_batches <= n) CHECK(moves == 0, "%d batches never share a stream, yet %d moves", n_batches, moves);
    printf("rotation: %d batches, %d in flight, %d steps, %d moves OK\n", n_batches, depth, steps, moves);
}

int main() {
    exhaustive();
    rotation(4, 3, 40);  // the streaming bench: depth + 1 batches
    rotation(3, 3, 40);  // resident: as many batches as streams — nobody moves
    rotation(3, 2, 40);
    rotation(2, 1, 40);
    rotation(5, 3, 40);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("stream lease ok\n");
    return 0;
}
