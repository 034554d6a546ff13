// vx_resources.hpp — the handles that own what the engine takes from the
// runtime (DESIGN.md §6 "Ownership"): DeviceMem, PinnedMem, Event, Stream and
// Stage.  Each is move-only, empty by default, and gives its resource back in
// reset(), which the destructor calls.  So a struct's members go in reverse
// declaration order: declare a stream after the memory and the events its
// work uses, and it is synchronized and destroyed before they are freed.
//
// The handles report failure and leave the error code and text to the caller.
// They reach the runtime only through vx_res::backend, defined once over HIP
// (vx_engine.hip); this header needs HIP's types alone, so a CPU program can
// include it and define the backend itself (tests/native/resources_check.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <sys/mman.h>

#include <cstdint>
#include <utility>

namespace vx_res {

namespace backend {
void* device_alloc(uint64_t bytes);  // NULL: failed
void device_free(void* p);
void* pinned_alloc(uint64_t bytes);  // NULL: failed
void pinned_free(void* p);
hipEvent_t event_create(unsigned flags);  // NULL: failed
void event_destroy(hipEvent_t e);
hipStream_t stream_create(unsigned flags, const int* priority);  // priority NULL: the default; NULL: failed
void stream_synchronize(hipStream_t s);
void stream_destroy(hipStream_t s);
bool stage_register(void* p, uint64_t bytes);  // pins a host mapping
void stage_unregister(void* p);
}  // namespace backend

// A byte block from alloc(bytes), given back with release(p).
template <void* (*alloc)(uint64_t), void (*release)(void*)>
class Block {
public:
    Block() = default;
    Block(Block&& o) noexcept : p_(std::exchange(o.p_, nullptr)), size_(std::exchange(o.size_, 0)) {}
    Block& operator=(Block&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            size_ = std::exchange(o.size_, 0);
        }
        return *this;
    }
    ~Block() { reset(); }
    void reset() {
        if (p_) release(p_);
        p_ = nullptr;
        size_ = 0;
    }
    explicit operator bool() const { return p_ != nullptr; }
    uint8_t* get() const { return p_; }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p_);
    }
    uint64_t size() const { return size_; }
    // At least `bytes`: nothing when the block already holds them, otherwise
    // the old block is freed and a new one allocated (contents are not kept;
    // it never shrinks).  false: the allocation failed and the handle is empty.
    bool reserve(uint64_t bytes) {
        if (size_ >= bytes) return true;
        reset();
        p_ = static_cast<uint8_t*>(alloc(bytes));
        size_ = p_ ? bytes : 0;
        return p_ != nullptr;
    }

private:
    uint8_t* p_ = nullptr;
    uint64_t size_ = 0;
};
using DeviceMem = Block<backend::device_alloc, backend::device_free>;
using PinnedMem = Block<backend::pinned_alloc, backend::pinned_free>;

class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    void reset() {
        if (e_) backend::event_destroy(e_);
        e_ = nullptr;
    }
    explicit operator bool() const { return e_ != nullptr; }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }  // where a runtime call takes the event
    // flags: hipEventDisableTiming, or hipEventDefault for a timed one
    bool make(unsigned flags) {
        reset();
        e_ = backend::event_create(flags);
        return e_ != nullptr;
    }

private:
    hipEvent_t e_ = nullptr;
};

class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) {
            reset();
            s_ = std::exchange(o.s_, nullptr);
        }
        return *this;
    }
    ~Stream() { reset(); }
    // Waits for the stream's work first: nothing queued on it may outlive the
    // memory and events declared before it.
    void reset() {
        if (s_) {
            backend::stream_synchronize(s_);
            backend::stream_destroy(s_);
        }
        s_ = nullptr;
    }
    explicit operator bool() const { return s_ != nullptr; }
    hipStream_t get() const { return s_; }
    operator hipStream_t() const { return s_; }  // where a runtime call or a launch takes the stream
    bool make(unsigned flags) { return set(backend::stream_create(flags, nullptr)); }
    bool make_with_priority(unsigned flags, int priority) { return set(backend::stream_create(flags, &priority)); }

private:
    bool set(hipStream_t s) {
        reset();
        s_ = s;
        return s_ != nullptr;
    }
    hipStream_t s_ = nullptr;
};

// A slot's pinned stage.  huge: an anonymous mapping aligned to 2 MiB with
// MADV_HUGEPAGE, faulted in, then registered, so the readers' O_DIRECT reads
// and the H2D copies touch 512x fewer page-table and IOMMU entries than with
// the pinned allocator's 4 KiB pages; where the mapping or its
// registration is refused, and without huge, pinned_alloc memory.
class Stage {
public:
    Stage() = default;
    Stage(Stage&& o) noexcept : p_(std::exchange(o.p_, nullptr)), map_(std::exchange(o.map_, 0)) {}
    Stage& operator=(Stage&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            map_ = std::exchange(o.map_, 0);
        }
        return *this;
    }
    ~Stage() { reset(); }
    void reset() {
        if (p_ && map_) {
            backend::stage_unregister(p_);
            munmap(p_, map_);
        } else if (p_) {
            backend::pinned_free(p_);
        }
        p_ = nullptr;
        map_ = 0;
    }
    explicit operator bool() const { return p_ != nullptr; }
    uint8_t* get() const { return p_; }
    uint64_t stage_map() const { return map_; }  // > 0: a registered mapping of this many bytes
    bool make(uint64_t bytes, bool huge) {
        reset();
        if (huge) map_huge(bytes);
        if (!p_) p_ = static_cast<uint8_t*>(backend::pinned_alloc(bytes));
        return p_ != nullptr;
    }

private:
    void map_huge(uint64_t bytes) {
        constexpr uint64_t kHuge = 2ull << 20;
        const uint64_t len = (bytes + kHuge - 1) / kHuge * kHuge;
        void* raw = mmap(nullptr, len + kHuge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (raw == MAP_FAILED) return;
        const uintptr_t r = reinterpret_cast<uintptr_t>(raw), a = (r + kHuge - 1) / kHuge * kHuge;
        if (a > r) munmap(raw, a - r);  // trim to the aligned [a, a + len)
        if (r + len + kHuge > a + len) munmap(reinterpret_cast<void*>(a + len), r + len + kHuge - (a + len));
        uint8_t* p = reinterpret_cast<uint8_t*>(a);
        (void)madvise(p, len, MADV_HUGEPAGE);  // a hint: 4 KiB pages where THP is off
        // A client that forks (hooks, helpers) must not turn the pinned pages
        // copy-on-write in the parent: the GPU keeps DMAing to the pinned page
        // while a write after the fork would move the parent to a new one.
        (void)madvise(p, len, MADV_DONTFORK);
        for (uint64_t o = 0; o < len; o += 4096) p[o] = 0;
        if (!backend::stage_register(p, len)) {
            munmap(p, len);
            return;
        }
        p_ = p;
        map_ = len;
    }
    uint8_t* p_ = nullptr;
    uint64_t map_ = 0;
};

}  // namespace vx_res
