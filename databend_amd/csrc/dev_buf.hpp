// dev_buf.hpp — Buf<T, Mem>: the one owner of a grow-only buffer of the C ABI's handles (the
// aggregation handle, the communicator, the scan context) and of their calls' temporaries.
//
// A Buf is a pointer, its capacity in elements and a destructor that frees it: move-only, empty
// after a move.  `Mem` says where the memory lives: DeviceMem (hipMalloc) and PinnedMem
// (hipHostMalloc) are the two shipped; MappedMem is PinnedMem with the flags of the one buffer
// kernels write.  Every way to grow either succeeds or leaves the buffer in a state its owner can
// go on with: {nullptr, 0} after a failed ensure, untouched after a failed grow_keep.  Nothing here synchronises on its own account except where a method says so, and the
// destructor frees without waiting: the owner drains its streams first (dbg_agg_destroy).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>

#include "../../include/dbgpu_agg.h"

int fail(int code, const std::string& msg);  // abi.hip: the code, with msg as dbg_last_error

inline int dev_alloc(void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(DBG_ERR_OOM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    return DBG_OK;
}

inline int mem_check(hipError_t e, const char* what) {
    return e == hipSuccess ? DBG_OK : fail(DBG_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

struct DeviceMem {
    static int alloc(void** p, size_t bytes) { return dev_alloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
    static int copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
        return mem_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
    }
    static int sync(hipStream_t s) { return mem_check(hipStreamSynchronize(s), "hipStreamSynchronize"); }
};

struct PinnedMem {
    static int alloc(void** p, size_t bytes) { return mem_check(hipHostMalloc(p, bytes, hipHostMallocDefault), "hipHostMalloc"); }
    static void free(void* p) { (void)hipHostFree(p); }
    static int sync(hipStream_t s) { return DeviceMem::sync(s); }
};

// pinned, mapped into the device's address space and coherent: kernels post results into it
struct MappedMem {
    static int alloc(void** p, size_t bytes) {
        if (hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return fail(DBG_ERR_OOM, "pinned");
        return DBG_OK;
    }
    static void free(void* p) { (void)hipHostFree(p); }
};

template <typename T, typename Mem = DeviceMem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    // the raw pointer, for kernel arguments and descriptor structs
    T* get() const { return p_; }
    operator T*() const { return p_; }
    uint64_t cap() const { return cap_; }  // elements

    // Frees what the buffer holds.
    void reset() {
        if (p_) Mem::free(p_);
        p_ = nullptr, cap_ = 0;
    }

    // Room for `need` elements, contents discarded: nothing happens while the buffer holds that
    // many; else it is freed and `alloc` (>= need) elements are allocated.
    int ensure_alloc(uint64_t need, uint64_t alloc) {
        if (p_ && need <= cap_) return DBG_OK;
        reset();
        void* p = nullptr;
        int rc = Mem::alloc(&p, alloc * sizeof(T));
        if (rc != DBG_OK) return rc;
        p_ = (T*)p, cap_ = alloc;
        return DBG_OK;
    }
    // ... allocating max(need, floor) elements
    int ensure(uint64_t need, uint64_t floor = 0) { return ensure_alloc(need, need > floor ? need : floor); }
    // ensure() of memory that work queued on `s` may still read (pinned staging behind an
    // asynchronous copy): the stream is drained before the old block is freed.
    int ensure_after(hipStream_t s, uint64_t need, uint64_t floor = 0) {
        if (p_ && need > cap_) {
            int rc = Mem::sync(s);
            if (rc != DBG_OK) return rc;
        }
        return ensure(need, floor);
    }
    // Grows to `alloc` elements keeping the first `used`: allocate, copy on `s`, wait for `s`,
    // free the old block.  A failed allocation leaves the buffer as it was.
    int grow_keep(uint64_t alloc, uint64_t used, hipStream_t s) {
        void* p = nullptr;
        int rc = Mem::alloc(&p, alloc * sizeof(T));
        if (rc != DBG_OK) return rc;
        Buf old(std::move(*this));
        p_ = (T*)p, cap_ = alloc;
        if (!old.p_) return DBG_OK;
        if (used) rc = Mem::copy(p_, old.p_, used * sizeof(T), s);
        if (rc == DBG_OK) rc = Mem::sync(s);  // the old block is freed when this returns
        return rc;
    }

private:
    T* p_ = nullptr;
    uint64_t cap_ = 0;
};

template <typename T>
using PinnedBuf = Buf<T, PinnedMem>;
