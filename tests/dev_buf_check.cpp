// Stand-alone check of Buf<T, Mem> (databend_amd/csrc/dev_buf.hpp) over a malloc-backed policy that
// counts what it hands out and can be told to fail: built with -fsanitize=address,undefined and run
// as a plain program by tests/test_dev_buf.py.  No device is touched: the shipped policies are never
// instantiated.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "dev_buf.hpp"

struct TestMem {
    static inline std::set<void*> live;
    static inline int allocs = 0, frees = 0, copies = 0, syncs = 0;
    static inline size_t last_bytes = 0;
    static inline bool fail_next = false;
    static int alloc(void** p, size_t bytes) {
        if (fail_next) {
            fail_next = false;
            return DBG_ERR_OOM;
        }
        *p = malloc(bytes ? bytes : 1);
        live.insert(*p);
        ++allocs;
        last_bytes = bytes;
        return DBG_OK;
    }
    static void free(void* p) {
        if (live.erase(p) != 1) {
            fprintf(stderr, "freed %p, which is not a live allocation\n", p);
            abort();
        }
        ::free(p);
        ++frees;
    }
    static int copy(void* dst, const void* src, size_t bytes, hipStream_t) {
        memcpy(dst, src, bytes);
        ++copies;
        return DBG_OK;
    }
    static int sync(hipStream_t) {
        ++syncs;
        return DBG_OK;
    }
};
using TBuf = Buf<uint32_t, TestMem>;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static int run() {
    using M = TestMem;
    {
        TBuf b;
        CHECK(b.get() == nullptr && b.cap() == 0 && !b);
        // the first ensure allocates max(need, floor) elements
        CHECK(b.ensure(10, 64) == DBG_OK);
        CHECK(M::allocs == 1 && M::frees == 0 && M::last_bytes == 64 * sizeof(uint32_t) && b.cap() == 64 && b.get());
        uint32_t* p0 = b;
        // at or below the capacity: nothing is allocated or freed
        CHECK(b.ensure(1, 64) == DBG_OK && b.ensure(64, 64) == DBG_OK && b.ensure(64) == DBG_OK);
        CHECK(M::allocs == 1 && M::frees == 0 && b.get() == p0 && b.cap() == 64);
        // above it: one free, one allocation of the requested size (the floor no longer matters)
        CHECK(b.ensure(65, 64) == DBG_OK);
        CHECK(M::allocs == 2 && M::frees == 1 && M::last_bytes == 65 * sizeof(uint32_t) && b.cap() == 65);
        // the size to allocate given outright
        CHECK(b.ensure_alloc(100, 125) == DBG_OK);
        CHECK(M::allocs == 3 && M::frees == 2 && M::last_bytes == 125 * sizeof(uint32_t) && b.cap() == 125);
        CHECK(b.ensure_alloc(125, 1000) == DBG_OK && M::allocs == 3);
        // a failed ensure leaves {nullptr, 0} (the old block freed once), and the next one succeeds
        M::fail_next = true;
        CHECK(b.ensure(500) == DBG_ERR_OOM);
        CHECK(b.get() == nullptr && b.cap() == 0 && M::allocs == 3 && M::frees == 3 && M::live.empty());
        CHECK(b.ensure(0) == DBG_OK);  // an empty buffer allocates even for no elements: the pointer is usable
        CHECK(b.get() && b.cap() == 0 && M::allocs == 4);
        CHECK(b.ensure(500) == DBG_OK && b.cap() == 500 && M::allocs == 5 && M::frees == 4);
        // ensure_after waits for the stream only when it is about to free a block
        CHECK(b.ensure_after(nullptr, 500, 1024) == DBG_OK && M::syncs == 0 && M::allocs == 5);
        CHECK(b.ensure_after(nullptr, 501, 1024) == DBG_OK && M::syncs == 1 && b.cap() == 1024 && M::frees == 5);
        TBuf fresh;
        CHECK(fresh.ensure_after(nullptr, 3, 1024) == DBG_OK && M::syncs == 1 && fresh.cap() == 1024);
    }
    CHECK(M::live.empty() && M::allocs == M::frees);

    {  // grow_keep
        TBuf b;
        CHECK(b.grow_keep(8, 0, nullptr) == DBG_OK && b.cap() == 8);  // from empty: no copy, no wait
        CHECK(M::copies == 0 && M::syncs == 1);
        for (uint32_t i = 0; i < 8; ++i) b[i] = 1000 + i;
        uint32_t* p0 = b;
        const int allocs0 = M::allocs, frees0 = M::frees;
        // a failed allocation leaves pointer, capacity and contents as they were
        M::fail_next = true;
        CHECK(b.grow_keep(16, 8, nullptr) == DBG_ERR_OOM);
        CHECK(b.get() == p0 && b.cap() == 8 && M::allocs == allocs0 && M::frees == frees0 && M::copies == 0);
        for (uint32_t i = 0; i < 8; ++i) CHECK(b[i] == 1000 + i);
        // success: the first `used` elements carried over, one copy, one wait, the old block freed
        CHECK(b.grow_keep(16, 5, nullptr) == DBG_OK);
        CHECK(b.cap() == 16 && M::allocs == allocs0 + 1 && M::frees == frees0 + 1 && M::copies == 1 && M::syncs == 2);
        CHECK(M::last_bytes == 16 * sizeof(uint32_t));
        for (uint32_t i = 0; i < 5; ++i) CHECK(b[i] == 1000 + i);
        // nothing used: no copy, still the wait before the old block goes
        CHECK(b.grow_keep(32, 0, nullptr) == DBG_OK && M::copies == 1 && M::syncs == 3 && b.cap() == 32);
    }
    CHECK(M::live.empty() && M::allocs == M::frees);

    {  // move: the source is left empty, the target's old block is freed
        TBuf a, b;
        CHECK(a.ensure(4) == DBG_OK && b.ensure(9) == DBG_OK);
        uint32_t* pa = a;
        const int frees0 = M::frees;
        TBuf c(std::move(a));
        CHECK(a.get() == nullptr && a.cap() == 0 && c.get() == pa && c.cap() == 4 && M::frees == frees0);
        b = std::move(c);
        CHECK(c.get() == nullptr && c.cap() == 0 && b.get() == pa && b.cap() == 4 && M::frees == frees0 + 1);
        TBuf& self = b;
        b = std::move(self);  // self-move keeps the block
        CHECK(b.get() == pa && b.cap() == 4);
        b.reset();
        CHECK(b.get() == nullptr && b.cap() == 0 && M::frees == frees0 + 2);
        CHECK(a.ensure(2) == DBG_OK && a.cap() == 2);  // a moved-from buffer is an empty one
    }
    CHECK(M::live.empty() && M::allocs == M::frees);

    {  // a vector that reallocates moves its buffers: every block is freed exactly once
        const int allocs0 = M::allocs, frees0 = M::frees;
        std::vector<TBuf> v;
        std::vector<uint32_t*> ptrs;
        for (int i = 0; i < 100; ++i) {
            TBuf b;
            CHECK(b.ensure(i + 1) == DBG_OK);
            b[0] = (uint32_t)i;
            ptrs.push_back(b);
            v.push_back(std::move(b));
        }
        CHECK(M::frees == frees0 && (int)M::live.size() == 100);
        for (int i = 0; i < 100; ++i) CHECK(v[i].get() == ptrs[i] && v[i][0] == (uint32_t)i && v[i].cap() == (uint64_t)i + 1);
        v.resize(40);
        CHECK(M::frees == frees0 + 60);
        v.clear();
        CHECK(M::allocs == allocs0 + 100 && M::frees == frees0 + 100);
    }
    CHECK(M::live.empty() && M::allocs == M::frees);
    return 0;
}

int main() {
    if (run()) return 1;
    printf("dev_buf ok: %d allocations, %d frees, 0 live\n", TestMem::allocs, TestMem::frees);
    return 0;
}
