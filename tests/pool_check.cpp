// Host check of the engine's activation pool and its owning handle (genpercept_amd/csrc/pool.h) over malloc / free; tests/test_pool_host.py
// builds it with AddressSanitizer + UBSan and runs it.  Every check is a plain `if (...) return fail(...)`; the sanitizers report a double
// free or a use after free in the handle itself, and a leak when the pool's destructor misses a buffer.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <stdexcept>
#include <utility>

#include "../genpercept_amd/csrc/pool.h"

namespace {

int n_malloc = 0, n_free = 0;
void* host_alloc(size_t bytes) {
    ++n_malloc;
    void* p = std::malloc(bytes);
    if (!p) throw std::runtime_error("malloc");
    return p;
}
void host_free(void* p) {
    ++n_free;
    std::free(p);
}

int fail(int line) {
    std::printf("pool_check: FAILED at line %d\n", line);
    return 1;
}
#define CHECK(c) \
    if (!(c)) return fail(__LINE__)

int times_free(const Pool& pool, void* p) {
    int n = 0;
    for (auto& kv : pool.free_list()) n += kv.second == p;
    return n;
}

// what an activation is: a tensor and the statistics that go with it
struct Pair {
    Pool::Buf data, stats;
};

constexpr size_t MiB = 1u << 20;

// 1. a released buffer is what the next alloc of the same size returns; sizes are rounded up to 256 bytes; total does not grow on reuse
int check_reuse() {
    Pool pool(host_alloc, host_free);
    void* first;
    {
        Pool::Buf a = pool.alloc(1000);
        first = a.get<void>();
        CHECK(first && pool.total == 1024 && pool.outstanding == 1 && pool.size_of(first) == 1024);
        CHECK(pool.free_list().empty());
    }
    CHECK(pool.outstanding == 0 && times_free(pool, first) == 1);
    Pool::Buf b = pool.alloc(1000);
    CHECK(b.get<char>() == first && pool.total == 1024 && pool.outstanding == 1 && pool.free_list().empty());
    Pool::Buf c = pool.alloc(1000);  // nothing free: a new buffer
    CHECK(c.get<void>() != first && pool.total == 2048 && pool.outstanding == 2);
    return 0;
}

// 2. the reuse bound: a request of n bytes takes a free buffer of 2 n + 1 MiB and leaves one of 2 n + 1 MiB + 256 alone
int check_bound() {
    const size_t n = 4096;
    {
        Pool pool(host_alloc, host_free);
        void* big = pool.alloc(2 * n + MiB).get<void>();  // (the temporary owner ends with the statement)
        CHECK(times_free(pool, big) == 1);
        Pool::Buf a = pool.alloc(n);
        CHECK(a.get<void>() == big && pool.total == 2 * n + MiB);
    }
    {
        Pool pool(host_alloc, host_free);
        void* big = pool.alloc(2 * n + MiB + 256).get<void>();
        Pool::Buf a = pool.alloc(n);
        CHECK(a.get<void>() != big && pool.total == 2 * n + MiB + 256 + n && times_free(pool, big) == 1);
        // lower_bound: a smaller free buffer is never taken
        void* small = pool.alloc(n - 256).get<void>();
        Pool::Buf b = pool.alloc(n);
        CHECK(b.get<void>() != small && b.get<void>() != big && times_free(pool, small) == 1);
    }
    return 0;
}

// 3. move construction and move assignment
int check_moves() {
    Pool pool(host_alloc, host_free);
    Pool::Buf a = pool.alloc(512);
    void* pa = a.get<void>();
    Pool::Buf b(std::move(a));
    CHECK(!a.get<void>() && b.get<void>() == pa && pool.outstanding == 1 && pool.free_list().empty());
    Pool::Buf c = pool.alloc(2048);
    void* pc = c.get<void>();
    CHECK(pool.outstanding == 2);
    c = std::move(b);  // releases what c held, once
    CHECK(!b.get<void>() && c.get<void>() == pa && pool.outstanding == 1 && times_free(pool, pc) == 1 && times_free(pool, pa) == 0);
    Pool::Buf empty;
    c = std::move(empty);  // assigning an empty owner releases too
    CHECK(!c.get<void>() && !empty.get<void>() && pool.outstanding == 0 && times_free(pool, pa) == 1 && times_free(pool, pc) == 1);
    Pool::Buf d;
    d = pool.alloc(512);  // into an empty owner: nothing to release
    CHECK(d.get<void>() == pa && pool.outstanding == 1 && pool.free_list().size() == 1);
    return 0;
}

// 4. reset() twice, and destruction after reset(), release once
int check_reset() {
    Pool pool(host_alloc, host_free);
    void* p;
    {
        Pool::Buf a = pool.alloc(256);
        p = a.get<void>();
        a.reset();
        CHECK(!a.get<void>() && pool.outstanding == 0 && times_free(pool, p) == 1);
        a.reset();
        CHECK(pool.outstanding == 0 && times_free(pool, p) == 1);
    }
    CHECK(pool.outstanding == 0 && times_free(pool, p) == 1 && pool.free_list().size() == 1);
    return 0;
}

// 5. a function that throws with buffers in hand leaves none outstanding and each on the free list once
std::set<void*> handed;
void throws_midway(Pool& pool) {
    Pool::Buf scratch[5];
    for (int i = 0; i < 5; ++i) {
        scratch[i] = pool.alloc(1024 * (size_t)(i + 1));
        handed.insert(scratch[i].get<void>());
    }
    Pair act{pool.alloc(8192), pool.alloc(256)};
    handed.insert(act.data.get<void>());
    handed.insert(act.stats.get<void>());
    Pair moved = std::move(act);
    if (pool.outstanding != 7) throw std::logic_error("outstanding");
    throw std::runtime_error("a stage failed");
}
int check_unwind() {
    Pool pool(host_alloc, host_free);
    bool caught = false;
    try {
        throws_midway(pool);
    } catch (const std::runtime_error&) {
        caught = true;
    }
    CHECK(caught && handed.size() == 7 && pool.outstanding == 0 && pool.free_list().size() == 7);
    for (void* p : handed) CHECK(times_free(pool, p) == 1);
    return 0;
}

// 6. a persistent buffer is not counted as outstanding and is not handed out again while held
int check_persistent() {
    Pool pool(host_alloc, host_free);
    Pool::Buf ws = pool.alloc_persistent(4096);
    void* pw = ws.get<void>();
    CHECK(pw && pool.outstanding == 0 && pool.total == 4096);
    {
        Pool::Buf a = pool.alloc(4096);
        CHECK(a.get<void>() != pw && pool.outstanding == 1);
    }
    CHECK(pool.outstanding == 0 && times_free(pool, pw) == 0);
    ws.reset();  // growing it: back to the free list, uncounted, then a larger one
    CHECK(pool.outstanding == 0 && times_free(pool, pw) == 1);
    ws = pool.alloc_persistent(3 * MiB);
    CHECK(ws.get<void>() != pw && pool.outstanding == 0);
    Pool::Buf moved = std::move(ws);  // the move keeps it uncounted
    moved.reset();
    CHECK(pool.outstanding == 0);
    return 0;
}

// 7. h = f(h): the allocation inside f cannot receive h's buffer, and h's old buffer is free afterwards
Pool::Buf next_layer(Pool& pool, const Pool::Buf& in, size_t bytes, void** got) {
    Pool::Buf out = pool.alloc(bytes);
    *got = out.get<void>();
    (void)in;
    return out;
}
int check_assign_from_self() {
    Pool pool(host_alloc, host_free);
    Pool::Buf h = pool.alloc(1024);
    void* old = h.get<void>();
    void* got = nullptr;
    h = next_layer(pool, h, 1024, &got);
    CHECK(got && got != old && h.get<void>() == got && times_free(pool, old) == 1 && pool.outstanding == 1);
    h = next_layer(pool, h, 1024, &got);  // the layer after that is the first to reuse it
    CHECK(got == old && pool.outstanding == 1 && pool.total == 2048);
    return 0;
}

}  // namespace

int main() {
    int (*const checks[])() = {check_reuse, check_bound, check_moves, check_reset, check_unwind, check_persistent, check_assign_from_self};
    for (auto c : checks)
        if (c()) return 1;
    if (n_malloc == 0 || n_free != n_malloc) return fail(__LINE__);  // every pool freed exactly what it allocated
    std::printf("ok\n");
    return 0;
}
