// tests/cpp/ndt_set_key_check.cpp — the host-side rules of a voxel-set target (csrc/ndt_set_key.hpp): the 64-bit key of target and
// voxel (round trip, range, linearity across the range boundary, never the empty marker), the per-scan words a pairs call forms from
// target_of, and the refusals an ingest decides before it touches the device. Stand-alone: compiled with and without
// -fsanitize=address,undefined by tests/test_ndt_pairs_abi.py.
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "ndt_set_key.hpp"

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

using namespace locgpu;

int main() {
    const unsigned long long kEmpty = ~0ull;  // kNdtEmpty of ndt_kernels.hpp
    // ---- the key: round trip at the corners of the range and of the target index
    const int edge[] = {-32767, -1, 0, 1, 32767};
    const uint32_t tg[] = {0u, 1u, 255u, 65534u};
    for (uint32_t t : tg)
        for (int x : edge)
            for (int y : edge)
                for (int z : edge) {
                    CHECK(ndt_set_key_in_range(x, y, z), "(%d, %d, %d) must be in range", x, y, z);
                    const unsigned long long k = ndt_set_pack(ndt_set_target_bits(t), x, y, z);
                    CHECK(k != kEmpty, "target %u voxel (%d, %d, %d) packs to the empty marker", t, x, y, z);
                    int t2, x2, y2, z2;
                    ndt_set_unpack(k, t2, x2, y2, z2);
                    CHECK((uint32_t)t2 == t && x2 == x && y2 == y && z2 == z, "round trip of target %u voxel (%d, %d, %d) gives %d (%d, %d, %d)", t, x, y, z, t2, x2, y2, z2);
                }
    CHECK(!ndt_set_coord_ok(32768) && !ndt_set_coord_ok(-32768) && ndt_set_coord_ok(32767) && ndt_set_coord_ok(-32767), "the range is -2^15 < k < 2^15");
    CHECK(!ndt_set_key_in_range(32768, 0, 0) && !ndt_set_key_in_range(0, -32768, 0) && !ndt_set_key_in_range(0, 0, 1 << 20), "out of range");
    CHECK(kNdtSetMaxTargets == 65535 && (ndt_set_target_bits(65535u) >> 48) == 0xFFFFull, "target 65535 is the one never given out");
    // keys of one target sort by (x, y, z); targets sort above voxels
    CHECK(ndt_set_pack(ndt_set_target_bits(3), -5, 7, 9) < ndt_set_pack(ndt_set_target_bits(3), -4, -7, -9), "x above y");
    CHECK(ndt_set_pack(ndt_set_target_bits(3), 2, 7, 9) < ndt_set_pack(ndt_set_target_bits(3), 2, 8, -9), "y above z");
    CHECK(ndt_set_pack(ndt_set_target_bits(3), 32767, 32767, 32767) < ndt_set_pack(ndt_set_target_bits(4), -32767, -32767, -32767), "target above x");
    // ---- linearity: centre + delta is the neighbour's key whenever the NEIGHBOUR is in range, also from a centre outside
    const int ox[7] = {0, -1, 1, 0, 0, 0, 0}, oy[7] = {0, 0, 0, 1, -1, 0, 0}, oz[7] = {0, 0, 0, 0, 0, -1, 1};
    const int centres[][3] = {{0, 0, 0}, {32768, 0, 0}, {-32768, 5, -7}, {12, 32768, 3}, {12, -32768, 3}, {1, 2, 32768}, {1, 2, -32768}, {32767, -32767, 32767},
                              {1048575, 0, 0}, {0, -1048575, 0}, {32768, 32768, 0}};
    for (uint32_t t : tg)
        for (const auto& c : centres) {
            const unsigned long long k0 = ndt_set_pack(ndt_set_target_bits(t), c[0], c[1], c[2]);
            int valid = 0;
            for (int j = 0; j < 7; ++j) {
                const int x = c[0] + ox[j], y = c[1] + oy[j], z = c[2] + oz[j];
                if (!ndt_set_key_in_range(x, y, z)) continue;
                ++valid;
                CHECK(k0 + ndt_set_delta(ox[j], oy[j], oz[j]) == ndt_set_pack(ndt_set_target_bits(t), x, y, z), "target %u centre (%d, %d, %d) probe %d", t, c[0], c[1], c[2], j);
            }
            if (c[0] == 32768 && c[1] == 0 && c[2] == 0) CHECK(valid == 1, "a centre one voxel outside on x has exactly one valid probe, not %d", valid);
            if (c[0] == 32768 && c[1] == 32768) CHECK(valid == 0, "a centre outside on two axes has no valid probe");
        }
    // ---- the per-scan words of a pairs call
    {
        std::vector<uint32_t> words{9u};
        std::vector<unsigned char> skip{9};
        std::string err;
        const int target_of[6] = {-1, 0, 1, 2, 5, 6};
        CHECK(pair_words(target_of, 6, 7, nullptr, words, skip, err), "valid target_of refused: %s", err.c_str());
        CHECK(words.size() == 6 && skip.size() == 6, "sizes");
        for (int i = 0; i < 6; ++i) {
            CHECK(skip[i] == (target_of[i] < 0 ? 1 : 0), "skip[%d]", i);
            CHECK(words[i] == (target_of[i] < 0 ? 0u : (uint32_t)target_of[i]), "words[%d] = %u", i, words[i]);
            if (!skip[i]) CHECK(ndt_set_target_bits(words[i]) == ((unsigned long long)target_of[i] << 48), "target bits of scan %d", i);
        }
        const uint32_t base[7] = {0, 10, 24, 30, 44, 50, 62};  // the ICP form: tree bases
        CHECK(pair_words(target_of, 6, 7, base, words, skip, err) && words[1] == 0 && words[2] == 10 && words[4] == 50 && words[5] == 62 && words[0] == 0 && skip[0] == 1, "bases");
        // refusals leave the outputs as they were and name the entry
        std::vector<uint32_t> w0 = words;
        std::vector<unsigned char> s0 = skip;
        const int too_big[6] = {-1, 0, 1, 2, 5, 7}, too_small[6] = {-2, 0, 1, 2, 5, 6};
        CHECK(!pair_words(too_big, 6, 7, nullptr, words, skip, err) && err.find("target_of[5] = 7") != std::string::npos, "target_of[5] = 7 of 7 targets: %s", err.c_str());
        CHECK(!pair_words(too_small, 6, 7, base, words, skip, err) && err.find("target_of[0] = -2") != std::string::npos, "target_of[0] = -2: %s", err.c_str());
        CHECK(words == w0 && skip == s0, "a refusal wrote its outputs");
        const int last[1] = {65534};
        CHECK(pair_words(last, 1, 65535, nullptr, words, skip, err) && words[0] == 65534u && ndt_set_pack(ndt_set_target_bits(words[0]), 32767, 32767, 32767) != kEmpty, "the last target");
    }
    // ---- what an ingest refuses before the device is touched
    {
        float a[9] = {0}, b[3] = {0};
        const void* pts[3] = {a, b, a};
        const size_t n[3] = {3, 1, 3};
        std::string err;
        CHECK(ndt_set_check_targets(pts, n, 3, 12, err), "valid set refused: %s", err.c_str());
        CHECK(!ndt_set_check_targets(nullptr, n, 3, 12, err) && err.find("NULL") != std::string::npos, "NULL pts");
        CHECK(!ndt_set_check_targets(pts, nullptr, 3, 12, err) && err.find("NULL") != std::string::npos, "NULL n");
        CHECK(!ndt_set_check_targets(pts, n, 0, 12, err) && !ndt_set_check_targets(pts, n, -4, 12, err) && !ndt_set_check_targets(pts, n, 65536, 12, err), "n_targets");
        CHECK(!ndt_set_check_targets(pts, n, 3, 11, err) && err.find("stride") != std::string::npos, "stride");
        const size_t with_empty[3] = {3, 0, 3};
        CHECK(!ndt_set_check_targets(pts, with_empty, 3, 12, err) && err.find("target 1") != std::string::npos, "an empty target is named: %s", err.c_str());
        const void* with_null[3] = {a, b, nullptr};
        CHECK(!ndt_set_check_targets(with_null, n, 3, 12, err) && err.find("target 2") != std::string::npos, "a NULL target is named: %s", err.c_str());
        const size_t huge[3] = {3, (size_t)kNdtSetMaxPoints, 3};
        CHECK(!ndt_set_check_targets(pts, huge, 3, 12, err) && err.find("target 1") != std::string::npos, "the size limit is named by target: %s", err.c_str());
        // 65535 targets are accepted
        std::vector<const void*> many(65535, a);
        std::vector<size_t> ones(65535, 1);
        CHECK(ndt_set_check_targets(many.data(), ones.data(), 65535, 16, err), "65535 targets: %s", err.c_str());
    }
    std::puts("ndt set key harness ok");
    return 0;
}
