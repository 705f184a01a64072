// loc_lib_amd/csrc/env.hpp — how the library reads its LOCGPU_* environment knobs (the table of all of them: DESIGN.md §11).
// Clamps and fall-backs stay with the caller, and so does "read once": keep the result in a function-local static.
#pragma once
#include <cstdlib>

namespace locgpu {

// atoi of the variable, `dflt` when it is not set
inline int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
// the variable is set, to whatever value
inline bool env_flag(const char* name) { return std::getenv(name) != nullptr; }

}  // namespace locgpu
