// Stand-alone host check of brx::DevBuf / brx::DevScratch (br_amd/csrc/brx_devbuf.hpp): the pool is replaced by malloc /
// free with a table of live blocks and a switch that fails the N-th allocation.  Built and run by test_devbuf_cpu.py with
// -fsanitize=address,undefined; exit status 0 = every check held and nothing leaked.
#include "../br_amd/csrc/brx_devbuf.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>

namespace {
std::map<void *, size_t> g_live; // block -> bytes asked for
int g_allocs = 0, g_frees = 0;   // calls into the "pool"
int g_fail_at = 0;               // fail the allocation that makes g_allocs reach this (0: never)
size_t g_last_bytes = 0;
std::string g_error;
int g_failed = 0;

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);               \
            g_failed++;                                                                            \
        }                                                                                          \
    } while (0)

struct A16 {
    uint64_t a, b;
};

#define TRY(expr)                                                                                  \
    do {                                                                                           \
        const int _s = (expr);                                                                     \
        if (_s != BRX_OK)                                                                          \
            return _s;                                                                             \
    } while (0)
} // namespace

namespace brx {
void set_error(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
hipError_t dev_alloc(void **out, size_t bytes)
{
    *out = nullptr;
    g_allocs++;
    g_last_bytes = bytes;
    if (g_fail_at && g_allocs == g_fail_at)
        return hipErrorOutOfMemory;
    *out = malloc(bytes ? bytes : 1);
    g_live[*out] = bytes;
    return hipSuccess;
}
hipError_t dev_free(void *p)
{
    g_frees++;
    if (!g_live.erase(p)) {
        fprintf(stderr, "dev_free of a block that is not live\n");
        g_failed++;
        return hipErrorInvalidValue;
    }
    free(p);
    return hipSuccess;
}
} // namespace brx

using brx::DevBuf;
using brx::DevScratch;

// growth, reuse within capacity and the failed growth, for one element type
template <typename T> static void check_reserve(const char *name)
{
    const int a0 = g_allocs, f0 = g_frees;
    {
        DevBuf<T> b;
        CHECK(b.get() == nullptr && b.cap() == 0 && !b);
        CHECK(b.reserve(100, 7, name) == BRX_OK);
        CHECK(g_allocs == a0 + 1 && g_frees == f0);
        CHECK(g_last_bytes == 107 * sizeof(T));
        CHECK(b.cap() == 107 && b.bytes() == 107 * sizeof(T));
        T *p = b;
        CHECK(p && g_live.count(p) && g_live[p] == 107 * sizeof(T));
        memset(p, 0x5a, 107 * sizeof(T)); // (ASan: the block really is that long)
        // within capacity: the same pointer, no call into the pool
        CHECK(b.reserve(100, 1000, name) == BRX_OK && b.reserve(107, 0, name) == BRX_OK && b.reserve(1, 1, name) == BRX_OK);
        CHECK(b.get() == p && g_allocs == a0 + 1 && g_frees == f0);
        // growth: the old block freed exactly once, exactly (need + headroom) * sizeof(T) asked for
        CHECK(b.reserve(108, 20, name) == BRX_OK);
        CHECK(g_allocs == a0 + 2 && g_frees == f0 + 1);
        CHECK(g_last_bytes == 128 * sizeof(T) && b.cap() == 128);
        CHECK(g_live.size() == 1 && g_live.count(b.get()));
        // a failed growth leaves the buffer empty, and says what and how much
        g_fail_at = g_allocs + 1;
        g_error.clear();
        CHECK(b.reserve(1000, 24, name) == BRX_ERR_NOMEM);
        g_fail_at = 0;
        CHECK(b.get() == nullptr && b.cap() == 0 && b.bytes() == 0);
        CHECK(g_frees == f0 + 2 && g_live.empty());
        CHECK(g_error.find(name) != std::string::npos);
        CHECK(g_error.find(std::to_string(1024 * sizeof(T))) != std::string::npos);
        // ... and the next, smaller reserve allocates again
        CHECK(b.reserve(10, 0, name) == BRX_OK);
        CHECK(b.get() != nullptr && b.cap() == 10 && g_last_bytes == 10 * sizeof(T));
        CHECK(g_allocs == a0 + 4);
    }
    CHECK(g_frees == f0 + 3 && g_live.empty()); // the destructor
}

static void check_bytes()
{
    DevBuf<uint32_t> b; // a headroom in bytes that is no whole number of elements
    CHECK(b.reserve_bytes(4 * 9, 4 * 9 / 8 + 256, "bytes") == BRX_OK);
    CHECK(g_last_bytes == 36 + 4 + 256 && b.bytes() == 296 && b.cap() == 74);
    const int a = g_allocs;
    CHECK(b.reserve_bytes(296, 0, "bytes") == BRX_OK && g_allocs == a);
    CHECK(b.reserve_bytes(297, 0, "bytes") == BRX_OK && g_allocs == a + 1 && g_last_bytes == 297);
}

static void check_moves()
{
    const int f0 = g_frees;
    DevBuf<uint32_t> a, b;
    CHECK(a.reserve(8, 0, "a") == BRX_OK && b.reserve(16, 0, "b") == BRX_OK);
    uint32_t *pa = a, *pb = b;
    // move construction: the source is left empty
    DevBuf<uint32_t> c(std::move(a));
    CHECK(c.get() == pa && c.cap() == 8 && a.get() == nullptr && a.cap() == 0 && g_frees == f0);
    // move assignment: the block the target held is freed, the source is left empty
    c = std::move(b);
    CHECK(c.get() == pb && c.cap() == 16 && b.get() == nullptr && b.cap() == 0);
    CHECK(g_frees == f0 + 1 && !g_live.count(pa) && g_live.count(pb));
    // swap
    CHECK(a.reserve(4, 0, "a") == BRX_OK);
    uint32_t *pa2 = a;
    a.swap(c);
    CHECK(a.get() == pb && a.cap() == 16 && c.get() == pa2 && c.cap() == 4 && g_frees == f0 + 1);
    // release: the caller owns the block, the buffer is empty and frees nothing
    uint32_t *r = a.release();
    CHECK(r == pb && a.get() == nullptr && a.cap() == 0 && g_live.count(pb));
    a.reset();
    CHECK(g_frees == f0 + 1);
    // adopt: frees what the buffer held, owns the block from then on
    c.adopt(r, 16);
    CHECK(c.get() == pb && c.cap() == 16 && g_frees == f0 + 2 && !g_live.count(pa2));
    c.adopt(nullptr, 5);
    CHECK(c.get() == nullptr && c.cap() == 0 && g_frees == f0 + 3 && g_live.empty());
    // reset frees now, once
    CHECK(c.reserve(3, 0, "c") == BRX_OK);
    c.reset();
    c.reset();
    CHECK(g_frees == f0 + 4 && g_live.empty());
}

static int scratch_user(bool fail_third)
{
    DevScratch ws;
    uint64_t *x = nullptr;
    uint8_t *y = nullptr;
    A16 *z = nullptr;
    TRY(ws.get(&x, 10));
    TRY(ws.get(&y, 0)); // (no empty blocks: one element)
    CHECK(g_last_bytes == 1);
    if (fail_third)
        g_fail_at = g_allocs + 1;
    TRY(ws.get(&z, 3));
    CHECK(g_last_bytes == 48 && g_live.size() == 3 && x && y && z);
    return BRX_OK;
}

static void check_scratch()
{
    const int f0 = g_frees;
    CHECK(scratch_user(false) == BRX_OK);
    CHECK(g_live.empty() && g_frees == f0 + 3);
    CHECK(scratch_user(true) == BRX_ERR_NOMEM); // the blocks it got before the failure go back too
    g_fail_at = 0;
    CHECK(g_live.empty() && g_frees == f0 + 5);
}

int main()
{
    check_reserve<uint8_t>("one byte");
    check_reserve<uint32_t>("four bytes");
    check_reserve<uint64_t>("eight bytes");
    check_reserve<A16>("sixteen bytes");
    check_bytes();
    check_moves();
    check_scratch();
    CHECK(g_live.empty());
    printf("devbuf_host: %d pool allocations, %d frees, %zu live blocks, %d failed checks\n", g_allocs, g_frees, g_live.size(), g_failed);
    return g_failed || !g_live.empty() ? 1 : 0;
}
