// prof.hpp — the event profiler's scope (dbg_prof_enable): HIP events around a launch.  The host
// units open a prof::Scope around what they launch; prof.hip keeps the state and the totals.
#pragma once
#include <hip/hip_runtime.h>

#pragma GCC visibility push(hidden)
namespace prof {
struct Scope {
    bool on;
    bool ext = false;  // a kernel launch stamped a / b itself (prof_ext_events)
    hipStream_t s;
    hipEvent_t a, b;
    const char* name;
    Scope* outer;
    Scope(const char* n, hipStream_t st);
    ~Scope();
};
}  // namespace prof
#pragma GCC visibility pop
