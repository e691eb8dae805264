"""DevBuf (yolo-nano_amd/csrc/yn_devbuf.h), the one owner of device memory, driven on the host: no GPU needed.

The library's growth paths (ensure_post, the evaluators' stores) only run when a buffer has to grow, and their failure paths only when
an allocation fails, which no GPU test may provoke.  A stand-alone driver compiled against the header with AddressSanitizer and UBSan
instantiates DevBuf over a malloc-backed allocator policy that counts its live blocks, checks every release against the block it was
given and can fail the k-th allocation or the copy.  Nothing is loaded into Python and the default (HIP) policy is never instantiated,
so the driver links without the HIP runtime."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo-nano_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DRIVER = r"""
#include "yn_devbuf.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct TA {                                     // malloc-backed policy: counts, checks each release, fails on request
    static inline std::map<void*, size_t> blocks;
    static inline long allocs = 0, releases = 0, fail_at = -1;     // fail_at: the allocation (counted from 0) that fails
    static inline bool fail_copy = false;
    static int alloc(void** p, size_t bytes)
    {
        if (allocs++ == fail_at) { *p = nullptr; return 2; }
        *p = std::malloc(bytes ? bytes : 1);
        CHECK(*p);
        blocks[*p] = bytes;
        return 0;
    }
    static void release(void* p, size_t bytes)
    {
        auto it = blocks.find(p);
        CHECK(it != blocks.end());              // a live block, released once
        CHECK(it->second == bytes);             // with the size it was allocated with
        blocks.erase(it);
        std::free(p);
        ++releases;
    }
    static int copy(void* dst, const void* src, size_t bytes, hipStream_t)
    {
        if (fail_copy) return 3;
        if (bytes) std::memcpy(dst, src, bytes);
        return 0;
    }
    static long live() { return (long)blocks.size(); }
};
template <typename T> using Buf = ynk::DevBuf<T, TA>;

// {nullptr, 0}, or a live block of at least cap() elements (all of them written: ASan sees an overstated capacity)
template <typename T> int holds(const Buf<T>& b)
{
    if (!b.get()) { CHECK(b.cap() == 0); return 0; }
    CHECK(b.cap() > 0);
    auto it = TA::blocks.find(b.get());
    CHECK(it != TA::blocks.end() && it->second >= b.cap() * sizeof(T));
    std::memset(b.get(), 0x5a, b.cap() * sizeof(T));
    return 1;
}

// the buffers of ensure_post: 8 per candidate, 10 per segment, the matrix, the prefilter's sync words
struct Post {
    Buf<float> f[4]; Buf<int32_t> i[4]; Buf<int32_t> seg[10]; Buf<unsigned long long> matrix, pre;
    static constexpr int COUNT = 20;
    int check(void** addr = nullptr) const      // every buffer satisfies the invariant; returns how many hold a block
    {
        int n = 0, k = 0;
        auto one = [&](const auto& b) { n += holds(b); if (addr) addr[k] = (void*)b.get(); ++k; };
        for (auto& b : f) one(b);
        for (auto& b : i) one(b);
        for (auto& b : seg) one(b);
        one(matrix); one(pre);
        CHECK(k == COUNT);
        return n;
    }
    int grow(size_t B, size_t N, size_t C, bool* moved)     // exact sizes, stops at the first failure (as ensure_post does)
    {
        const size_t need = B * N, need_seg = B * (C + 1);
        int rc = 0;
        auto take = [&](auto& b, size_t n) { if (!rc) rc = b.reserve(n, 0, moved); };
        take(f[0], need * 4); take(f[1], need); take(i[0], need); take(i[1], need); take(i[2], need); take(f[2], need * 4); take(i[3], need); take(f[3], need * 4);
        for (auto& b : seg) take(b, need_seg);
        take(matrix, B * 37); take(pre, B * 5 + 64);
        return rc;
    }
    bool covers(size_t B, size_t N, size_t C) const
    {
        bool ok = f[0].cap() >= B * N * 4 && f[1].cap() >= B * N && f[2].cap() >= B * N * 4 && f[3].cap() >= B * N * 4 && matrix.cap() >= B * 37 && pre.cap() >= B * 5 + 64;
        for (auto& b : i) ok = ok && b.cap() >= B * N;
        for (auto& b : seg) ok = ok && b.cap() >= B * (C + 1);
        return ok;
    }
};

static void grouped_growth_under_failure()
{
    for (int start = 0; start < 2; ++start)                 // from empty buffers, and from a smaller set that is live
        for (int k = 0; k < Post::COUNT; ++k) {
            CHECK(TA::live() == 0);
            {
                Post p;
                bool moved = false;
                if (start) { CHECK(p.grow(1, 100, 5, &moved) == 0 && moved && p.check() == Post::COUNT); }
                void *before[Post::COUNT], *after[Post::COUNT];
                p.check(before);
                moved = false;
                TA::fail_at = TA::allocs + k;
                CHECK(p.grow(3, 100, 5, &moved) != 0);
                TA::fail_at = -1;
                const int held = p.check(after);            // each buffer: empty or whole
                CHECK(TA::live() == held);                  // nothing leaked, nothing counted twice
                CHECK(held == (start ? Post::COUNT - 1 : k));   // the failed one is empty, the ones behind it keep their old block
                bool changed = false;
                for (int j = 0; j < Post::COUNT; ++j) changed = changed || before[j] != after[j];
                CHECK(moved == changed);                    // the caller drops its graphs exactly when an address changed
                CHECK(start ? moved : moved == (k > 0));
                CHECK(!p.covers(3, 100, 5));
                CHECK(p.grow(3, 100, 5, &moved) == 0);       // the retry goes through
                CHECK(p.check() == Post::COUNT && TA::live() == Post::COUNT && p.covers(3, 100, 5));
                moved = false;
                p.check(before);
                CHECK(p.grow(2, 100, 5, &moved) == 0 && !moved);     // a smaller batch afterwards changes nothing
                p.check(after);
                CHECK(std::memcmp(before, after, sizeof before) == 0);
            }
            CHECK(TA::live() == 0);
        }
    std::printf("PASS grouped_growth_under_failure\n");
}

static void keeping_growth()
{
    {
        Buf<int32_t> b;
        bool moved = false;
        CHECK(b.reserve_keep(100, 0, nullptr, 4096, &moved) == 0 && moved && b.cap() == 4096);      // doubling from the call's first size
        for (int j = 0; j < 4096; ++j) b[j] = j * 7 + 1;
        int32_t* old = b.get();
        moved = false;
        CHECK(b.reserve_keep(4097, 4096, nullptr, 4096, &moved) == 0 && moved && b.cap() == 8192 && b.get() != old);
        for (int j = 0; j < 4096; ++j) CHECK(b[j] == j * 7 + 1);
        CHECK(TA::live() == 1 && holds(b) == 1);
        for (int j = 0; j < 8192; ++j) b[j] = -j;
        // the allocation fails: the old block and its contents stay
        old = b.get(); moved = false;
        TA::fail_at = TA::allocs;
        CHECK(b.reserve_keep(8193, 8192, nullptr, 4096, &moved) != 0 && !moved);
        TA::fail_at = -1;
        CHECK(b.get() == old && b.cap() == 8192 && TA::live() == 1);
        for (int j = 0; j < 8192; ++j) CHECK(b[j] == -j);
        // the copy fails: the same, and the new block is released
        TA::fail_copy = true;
        CHECK(b.reserve_keep(8193, 8192, nullptr, 4096, &moved) != 0 && !moved);
        TA::fail_copy = false;
        CHECK(b.get() == old && b.cap() == 8192 && TA::live() == 1);
        for (int j = 0; j < 8192; ++j) CHECK(b[j] == -j);
        CHECK(b.reserve_keep(20000, 8192, nullptr, 4096, &moved) == 0 && moved && b.cap() == 32768);
        for (int j = 0; j < 8192; ++j) CHECK(b[j] == -j);
        // the other rules: exact, and doubling from 1
        Buf<double> e, d;
        CHECK(e.reserve_keep(1000, 0, nullptr) == 0 && e.cap() == 1000);
        CHECK(d.reserve(5, 1) == 0 && d.cap() == 8 && d.reserve(9, 1) == 0 && d.cap() == 16 && d.reserve(3000) == 0 && d.cap() == 3000);
        // a dropping growth that fails leaves the buffer empty, not dangling
        TA::fail_at = TA::allocs;
        CHECK(d.reserve(3001) != 0 && d.get() == nullptr && d.cap() == 0);
        TA::fail_at = -1;
        CHECK(TA::live() == 2);
    }
    CHECK(TA::live() == 0);
    std::printf("PASS keeping_growth\n");
}

static void noop_growth()
{
    {
        Buf<float> b;
        bool moved = false;
        CHECK(b.reserve(0, 0, &moved) == 0 && !moved && b.get() == nullptr);
        CHECK(b.reserve(64, 0, &moved) == 0 && moved);
        float* p = b.get();
        const long allocs = TA::allocs;
        moved = false;
        CHECK(b.reserve(64, 0, &moved) == 0 && b.reserve(10, 1, &moved) == 0 && b.reserve_keep(64, 64, nullptr, 4096, &moved) == 0 &&
              b.reserve_keep(1, 1, nullptr, 0, &moved) == 0);
        CHECK(!moved && b.get() == p && b.cap() == 64 && TA::allocs == allocs);
        float* q = b;                                       // the conversion launch sites use
        CHECK(q == p);
    }
    CHECK(TA::live() == 0);
    std::printf("PASS noop_growth\n");
}

struct Two { Buf<float> a; Buf<int32_t> b; int tag = 0; };

static void relocation()
{
    static_assert(std::is_nothrow_move_constructible<Two>::value && !std::is_copy_constructible<Two>::value, "vector relocates by moving");
    const long allocs = TA::allocs, releases = TA::releases;
    {
        std::vector<Two> v;
        size_t reallocations = 0, cap = v.capacity();
        for (int j = 0; j < 100; ++j) {
            Two t;
            t.tag = j;
            CHECK(t.a.reserve(j + 1) == 0 && t.b.reserve(2 * j + 1) == 0);
            t.a[j] = (float)j;
            v.push_back(std::move(t));
            if (v.capacity() != cap) { ++reallocations; cap = v.capacity(); }
        }
        CHECK(reallocations >= 4);
        CHECK(TA::live() == 200 && TA::releases == releases);       // moving released nothing
        for (int j = 0; j < 100; ++j) CHECK(v[j].tag == j && v[j].a.cap() == (size_t)j + 1 && v[j].a[j] == (float)j && holds(v[j].a) && holds(v[j].b));
        v.clear();
        CHECK(TA::live() == 0);
    }
    CHECK(TA::allocs - allocs == 200 && TA::releases - releases == 200);     // each block exactly once
    std::printf("PASS relocation\n");
}

static void moves()
{
    {
        Buf<int32_t> a, b;
        CHECK(a.reserve(10) == 0 && b.reserve(20) == 0);
        int32_t* pb = b.get();
        const long releases = TA::releases;
        a = std::move(b);                                   // the target's old block goes
        CHECK(TA::releases == releases + 1 && TA::live() == 1);
        CHECK(a.get() == pb && a.cap() == 20 && b.get() == nullptr && b.cap() == 0);
        Buf<int32_t> c(std::move(a));
        CHECK(c.get() == pb && c.cap() == 20 && a.get() == nullptr && a.cap() == 0 && TA::live() == 1);
        Buf<int32_t>& self = c;
        c = std::move(self);                                // self-assignment keeps the block
        CHECK(c.get() == pb && c.cap() == 20 && TA::live() == 1);
        c.reset();
        CHECK(c.get() == nullptr && c.cap() == 0 && TA::live() == 0);
        c.reset();
    }
    CHECK(TA::live() == 0);
    std::printf("PASS moves\n");
}

int main()
{
    grouped_growth_under_failure();
    keeping_growth();
    noop_growth();
    relocation();
    moves();
    CHECK(TA::live() == 0);
    std::printf("DONE\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver_output():
    d = tempfile.mkdtemp(prefix="yn_devbuf_")
    src, exe = os.path.join(d, "devbuf.cpp"), os.path.join(d, "devbuf")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call([CXX] + FLAGS + ["-I", CSRC, src, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), "driver failed (%d)\n%s\n%s" % (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.split("\n")
    assert "DONE" in lines
    return lines


@pytest.mark.parametrize("check", ["grouped_growth_under_failure", "keeping_growth", "noop_growth", "relocation", "moves"])
def test_devbuf(driver_output, check):
    assert "PASS " + check in driver_output
