// prof.hip — profiling: HIP events around every launch (dbg_prof_enable).  Holds the profiler's
// state, prof::Scope's two ends (prof.hpp), the hooks the kernel units declare for themselves
// (prof_ext_events, prof_scope_begin / prof_scope_end) and the dbg_prof_* entry points with the
// marker kernel.  Which launches are timed is up to the units that open the scopes.
#include "abi_internal.hpp"

namespace prof {
struct Pending {
    std::string name;
    hipEvent_t a, b;
};
static std::mutex mu;
static bool enabled = false;
static std::vector<Pending> pending;
static std::vector<hipEvent_t> free_events;  // pooled: hipEventCreate is not free
static std::vector<std::pair<std::string, std::pair<double, uint64_t>>> totals;

static hipEvent_t get_event() {
    std::lock_guard<std::mutex> g(mu);
    if (!free_events.empty()) {
        hipEvent_t e = free_events.back();
        free_events.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

static void resolve_locked() {
    for (auto& p : pending) {
        float ms = 0;
        (void)hipEventSynchronize(p.b);
        (void)hipEventElapsedTime(&ms, p.a, p.b);
        free_events.push_back(p.a);
        free_events.push_back(p.b);
        bool found = false;
        for (auto& t : totals)
            if (t.first == p.name) {
                t.second.first += ms;
                t.second.second += 1;
                found = true;
                break;
            }
        if (!found) totals.push_back({p.name, {(double)ms, 1}});
    }
    pending.clear();
}

static thread_local Scope* cur = nullptr;  // the innermost open scope of this thread
Scope::Scope(const char* n, hipStream_t st) : on(enabled), s(st), name(n), outer(cur) {
    if (on) {
        a = get_event();
        b = get_event();
        (void)hipEventRecord(a, s);
        cur = this;
    }
}
Scope::~Scope() {
    if (on) {
        cur = outer;
        if (!ext) (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> g(mu);
        pending.push_back({name, a, b});
    }
}
}  // namespace prof

// A kernel that is the timed work of the innermost open scope: launched with
// hipExtLaunchKernelGGL and these two events, they are stamped at the kernel's own start and end
// (what rocprofv3 reports), not at the stream's event packets around it.  The scope then measures
// that kernel alone.
bool prof_ext_events(hipEvent_t* a, hipEvent_t* b) {
    prof::Scope* c = prof::cur;
    if (!c || !c->on || c->ext) return false;
    c->ext = true;
    *a = c->a;
    *b = c->b;
    return true;
}

// the same HIP-event scopes for the other translation units (scan.hip)
void* prof_scope_begin(const char* name, hipStream_t s) { return prof::enabled ? new prof::Scope(name, s) : nullptr; }
void prof_scope_end(void* p) { delete (prof::Scope*)p; }

__global__ void dbg_marker_kernel() {}

extern "C" {
int dbg_prof_enable(int on) {
    std::lock_guard<std::mutex> g(prof::mu);
    prof::enabled = on != 0;
    return DBG_OK;
}
int dbg_prof_reset(void) {
    std::lock_guard<std::mutex> g(prof::mu);
    prof::resolve_locked();
    prof::totals.clear();
    return DBG_OK;
}
int dbg_prof_get(int i, const char** name, double* total_ms, uint64_t* launches) {
    std::lock_guard<std::mutex> g(prof::mu);
    prof::resolve_locked();
    if (i < 0 || (size_t)i >= prof::totals.size()) return DBG_ERR_INVALID;
    *name = prof::totals[i].first.c_str();
    *total_ms = prof::totals[i].second.first;
    *launches = prof::totals[i].second.second;
    return DBG_OK;
}
int dbg_prof_marker(void* stream) {
    hipLaunchKernelGGL(dbg_marker_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}
}  // extern "C"
