// tests/cpp/ndt_key_check.cpp — the key rules of the NDT voxel tables (csrc/ndt_key.hpp, csrc/ndt_set_key.hpp) on the host: the packed
// key round trip at the edges of the ±2^20 range, never the empty marker, linear in the coordinates; then, for every line
// "x y z cap" or "x y z target cap" on standard input, one line of output
//     key <packed key, decimal> h32 <ndt_hash32 first slot> h64 <ndt_hash first slot>
// with the key ndt_pack's for four numbers and ndt_set_pack's under `target` for five — what tests/ndt_table_cases.py restates in numpy
// and tests/test_ndt_table_cases_ref.py compares. Stand-alone: compiled with and without -fsanitize=address,undefined by that test.
#include <cstdio>
#include <cstdint>
#include "ndt_key.hpp"
#include "ndt_set_key.hpp"

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

using namespace locgpu;

static void unpack(unsigned long long k, int& x, int& y, int& z) {  // the rule of ndt_dump_kernel / inc_ndt_dump
    x = (int)((k >> 42) & 0x1FFFFF) - kNdtBias;
    y = (int)((k >> 21) & 0x1FFFFF) - kNdtBias;
    z = (int)(k & 0x1FFFFF) - kNdtBias;
}

int main() {
    static_assert(kNdtEmpty == ~0ull && kNdtBias == (1 << 20), "the constants the numpy restatement carries");
    // ---- round trip at the edges of the range
    const int edge[] = {-1048575, -1048574, -1, 0, 1, 1048574, 1048575};
    for (int x : edge)
        for (int y : edge)
            for (int z : edge) {
                CHECK(ndt_key_in_range(x, y, z), "(%d, %d, %d) must be in range", x, y, z);
                const unsigned long long k = ndt_pack(x, y, z);
                CHECK(k != kNdtEmpty && (k >> 63) == 0, "voxel (%d, %d, %d) packs to the empty marker or past 63 bits", x, y, z);
                int x2, y2, z2;
                unpack(k, x2, y2, z2);
                CHECK(x2 == x && y2 == y && z2 == z, "round trip of (%d, %d, %d) gives (%d, %d, %d)", x, y, z, x2, y2, z2);
            }
    CHECK(!ndt_key_in_range(1048576, 0, 0) && !ndt_key_in_range(0, -1048576, 0) && !ndt_key_in_range(0, 0, 1048576) && !ndt_key_in_range(-1048576, -1048576, -1048576),
          "the range is -2^20 < k < 2^20");
    // keys sort by (x, y, z); a face neighbour's key is the centre's ± one constant (what ndt_accum_kernel adds)
    CHECK(ndt_pack(-5, 7, 9) < ndt_pack(-4, -7, -9) && ndt_pack(2, 7, 9) < ndt_pack(2, 8, -9), "x above y above z");
    const int ox[7] = {0, -1, 1, 0, 0, 0, 0}, oy[7] = {0, 0, 0, 1, -1, 0, 0}, oz[7] = {0, 0, 0, 0, 0, -1, 1};
    const int centres[][3] = {{0, 0, 0}, {17, -3, 160}, {-1048574, 1048574, 0}, {1048574, -1048574, -1048574}};
    for (const auto& c : centres)
        for (int j = 0; j < 7; ++j) {
            const long long delta = (long long)ox[j] * (1ll << 42) + (long long)oy[j] * (1ll << 21) + (long long)oz[j];
            CHECK(ndt_pack(c[0], c[1], c[2]) + (unsigned long long)delta == ndt_pack(c[0] + ox[j], c[1] + oy[j], c[2] + oz[j]), "centre (%d, %d, %d) probe %d", c[0], c[1], c[2], j);
        }
    // the hashes stay below the capacity and use its low bits only
    for (size_t cap = 1; cap <= ((size_t)1 << 26); cap <<= 1) {
        const unsigned long long k = ndt_pack(12, -7, 160);
        CHECK(ndt_hash(k, cap - 1) < cap && ndt_hash32(k, cap - 1) < cap, "a first slot beyond the table of %zu slots", cap);
        CHECK(ndt_hash(k, cap - 1) == (ndt_hash(k, ~(size_t)0) & (cap - 1)) && ndt_hash32(k, cap - 1) == (ndt_hash32(k, ~(size_t)0) & (cap - 1)), "low bits, %zu slots", cap);
    }
    // ---- the queries
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        long long v[5];
        const int n = std::sscanf(line, "%lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4]);
        if (n <= 0) continue;  // an empty line
        CHECK(n == 4 || n == 5, "a line of %d numbers: %s", n, line);
        const long long cap = v[n - 1];
        CHECK(cap >= 1 && cap <= (1ll << 40) && (cap & (cap - 1)) == 0, "capacity %lld is not a power of two", cap);
        const int x = (int)v[0], y = (int)v[1], z = (int)v[2];
        unsigned long long key;
        if (n == 4) {
            CHECK(ndt_key_in_range(x, y, z), "(%d, %d, %d) is outside the key range", x, y, z);
            key = ndt_pack(x, y, z);
        } else {
            CHECK(ndt_set_key_in_range(x, y, z) && v[3] >= 0 && v[3] < kNdtSetMaxTargets, "target %lld voxel (%d, %d, %d) is outside the set's range", v[3], x, y, z);
            key = ndt_set_pack(ndt_set_target_bits((uint32_t)v[3]), x, y, z);
        }
        std::printf("key %llu h32 %zu h64 %zu\n", key, ndt_hash32(key, (size_t)cap - 1), ndt_hash(key, (size_t)cap - 1));
    }
    std::puts("ndt key harness ok");
    return 0;
}
