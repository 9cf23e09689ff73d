// The binary reads and writes of the stand-alone check programs (tests/*_check.cpp): n items of `size` bytes each, true when all of them
// came through.  n = 0 is no access at all: an empty std::vector's data() may be null, and fread / fwrite take no null pointer.
#pragma once
#include <cstddef>
#include <cstdio>

static inline bool get(void* p, size_t size, size_t n, FILE* f) { return n == 0 || std::fread(p, size, n, f) == n; }
static inline bool put(const void* p, size_t size, size_t n, FILE* f) { return n == 0 || std::fwrite(p, size, n, f) == n; }
