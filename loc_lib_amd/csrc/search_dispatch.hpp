// loc_lib_amd/csrc/search_dispatch.hpp — run-time depth and k → the compile-time shapes of the search kernels, written once for
// icp_search.hip and icp_search_pairs.hip.
#pragma once
#include <type_traits>
#include <utility>

namespace locgpu {

// depth → the compile-time stack rows D ∈ {32, 40, 64} of the kernels: f(integral_constant<int, D>). False above 64 (no such kernel).
constexpr int kMaxSearchDepth = 64;
template <class F>
static bool with_depth(int depth, F&& f) {
    if (depth <= 32) f(std::integral_constant<int, 32>{});
    else if (depth <= 40) f(std::integral_constant<int, 40>{});
    else if (depth <= kMaxSearchDepth) f(std::integral_constant<int, 64>{});
    else return false;
    return true;
}
// k → the compile-time result-set size: f(integral_constant<int, K>), whose verdict is returned. The search stage has kernels for
// exactly k = 1 and k = 5; launch_knn_query (UP_TO) takes the next of {1, 5, 8}. False when there is none.
template <bool UP_TO, class F>
static bool with_k(int k, F&& f) {
    if (k == 1) return f(std::integral_constant<int, 1>{});
    if (UP_TO ? k <= 5 : k == 5) return f(std::integral_constant<int, 5>{});
    if constexpr (UP_TO)
        if (k <= 8) return f(std::integral_constant<int, 8>{});
    return false;
}

}  // namespace locgpu
