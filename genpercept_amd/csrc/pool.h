// The engine's activation pool and the handle that owns one of its buffers.  No HIP in here: the device allocator comes in as two function
// pointers (the engine passes hipMalloc / hipFree wrappers), so tests/pool_check.cpp runs the same code over malloc under a sanitizer.
//
// Buffers are recycled in stream order: a released buffer goes to the next alloc that fits, which is only safe within one stream (engine.hip:
// check_ready fences a change of stream).  The pool never returns memory before it is destroyed; `total` is its high-water mark.
#pragma once

#include <cstddef>
#include <map>
#include <unordered_map>
#include <utility>

class Pool {
public:
    using AllocFn = void* (*)(size_t bytes);  // throws when it cannot allocate
    using FreeFn = void (*)(void*);

    // Move-only owner of one pool buffer: the buffer goes back to the pool when the owner ends, or at reset().
    class Buf {
    public:
        Buf() = default;
        Buf(Buf&& o) noexcept : pool_(o.pool_), p_(std::exchange(o.p_, nullptr)), counted_(o.counted_) {}
        Buf& operator=(Buf&& o) noexcept {  // takes the new value first, then releases what it overwrites (h = f(h): f never receives h's buffer)
            Buf old(std::move(*this));
            pool_ = o.pool_; p_ = std::exchange(o.p_, nullptr); counted_ = o.counted_;
            return *this;
        }
        Buf(const Buf&) = delete;
        Buf& operator=(const Buf&) = delete;
        ~Buf() { reset(); }
        void reset() {
            if (p_) pool_->release(std::exchange(p_, nullptr), counted_);
        }
        template <typename T>
        T* get() const { return static_cast<T*>(p_); }

    private:
        friend class Pool;
        Buf(Pool* pool, void* p, bool counted) : pool_(pool), p_(p), counted_(counted) {}
        Pool* pool_ = nullptr;
        void* p_ = nullptr;
        bool counted_ = true;
    };

    Pool(AllocFn a, FreeFn f) : alloc_fn_(a), free_fn_(f) {}
    Pool(const Pool&) = delete;
    Pool& operator=(const Pool&) = delete;
    ~Pool() {  // every Buf must have ended before its pool does
        for (auto& kv : size_) free_fn_(kv.first);
    }

    Buf alloc(size_t bytes) {
        void* p = take(bytes);
        ++outstanding;
        return Buf(this, p, true);
    }
    // a buffer its owner keeps across calls: not part of a call's outstanding set
    Buf alloc_persistent(size_t bytes) { return Buf(this, take(bytes), false); }

    size_t total = 0;     // every byte ever allocated
    int outstanding = 0;  // buffers handed out by alloc() and not yet returned: zero between the engine's calls

    // (read-only views for the host test)
    const std::multimap<size_t, void*>& free_list() const { return free_; }
    size_t size_of(void* p) const { return size_.at(p); }

private:
    void* take(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        auto it = free_.lower_bound(bytes);
        void* p = nullptr;
        if (it != free_.end() && it->first <= bytes * 2 + (1u << 20)) {
            p = it->second;
            free_.erase(it);
        } else {
            p = alloc_fn_(bytes);
            size_[p] = bytes;
            total += bytes;
        }
        return p;
    }
    void release(void* p, bool counted) {
        free_.insert({size_.at(p), p});
        if (counted) --outstanding;
    }
    AllocFn alloc_fn_;
    FreeFn free_fn_;
    std::multimap<size_t, void*> free_;
    std::unordered_map<void*, size_t> size_;
};
