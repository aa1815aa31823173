// The buffer owner of csrc/pcabi_hostdev.h on the CPU: Owned over a fake memory policy that counts
// live blocks and fails the k-th allocation on request. Built with -fsanitize=address,undefined as a
// program of its own (tests/test_hostdev_cpu.py); a failed check prints its line and exits 1.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../custom_porechop_abi_amd/csrc/pcabi_hostdev.h"
#include "../custom_porechop_abi_amd/csrc/pcabi_scratch.h"

using pcabi_internal::holds;
using pcabi_internal::Owned;
using pcabi_internal::ScratchOf;

namespace {

constexpr int kNoMemory = -77;   // what the fake returns where the real policies return a fail() code

struct Fake {
    static int live, peak, allocs, frees, fail_at;   // fail_at: the number of the allocation that fails (1-based), 0 = none
    static int alloc(void **p, size_t n) {
        if (++allocs == fail_at) return kNoMemory;
        *p = std::malloc(n ? n : 1);
        peak = std::max(peak, ++live);
        return 0;
    }
    static void free(void *p) {
        std::free(p);
        --live;
        ++frees;
    }
    static void reset(int fail = 0) { live = peak = allocs = frees = 0, fail_at = fail; }
};
int Fake::live = 0, Fake::peak = 0, Fake::allocs = 0, Fake::frees = 0, Fake::fail_at = 0;

using Buf = Owned<Fake>;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("line %d: %s\n", __LINE__, #cond);                \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

// a stage in small: three slots' worth of buffers reserved in sequence, as the stage_reserve functions do
struct Three {
    Buf a, b;
    Owned<Fake, int64_t> c;
    bool kept(int64_t bytes, int64_t blocks) const { return holds(a, bytes + 16, b, bytes + 16, c, blocks + 1); }
    int reserve(int64_t bytes, int64_t blocks) {
        if (kept(bytes, blocks)) return 0;
        a.release(), b.release(), c.release();
        if (int rc = a.reserve(bytes + 16, bytes + 16)) return rc;
        if (int rc = b.reserve(bytes + 16, bytes + 16)) return rc;
        return c.reserve(blocks + 1, blocks + 1);
    }
};

}  // namespace

int main() {
    {   // 1. within the capacity: no allocation, the same pointer
        Fake::reset();
        Buf b;
        CHECK(b.p == nullptr && b.cap == 0 && b.reserve(0, 64) == 0 && Fake::allocs == 0);
        CHECK(b.reserve(100, 150) == 0 && b.cap == 150 && Fake::allocs == 1);
        uint8_t *p = b;
        p[149] = 1;
        CHECK(b.reserve(150, 999) == 0 && b.reserve(1, 1) == 0 && b.p == p && b.cap == 150 && Fake::allocs == 1);
        // 2. growth frees first: one owner never has two live blocks
        CHECK(b.reserve(151, 300) == 0 && b.cap == 300 && Fake::allocs == 2 && Fake::frees == 1 && Fake::peak == 1);
        b[299] = 2;
        Owned<Fake, int64_t> w;   // the capacity counts elements
        CHECK(w.reserve(10, 10) == 0 && w.cap == 10);
        w[9] = -1;
    }
    CHECK(Fake::live == 0 && Fake::frees == Fake::allocs);
    {   // 3. a failed reserve leaves {nullptr, 0}; the same reserve again allocates and succeeds
        Fake::reset(2);
        Buf b;
        CHECK(b.reserve(10, 10) == 0);
        CHECK(b.reserve(20, 30) == kNoMemory && b.p == nullptr && b.cap == 0 && Fake::live == 0 && Fake::frees == 1);
        CHECK(!holds(b, 20) && !holds(b, 1) && holds(b, 0));
        CHECK(b.reserve(20, 30) == 0 && b.p != nullptr && b.cap == 30 && Fake::allocs == 3 && Fake::live == 1);
    }
    CHECK(Fake::live == 0);
    {   // 4. moves, release() and destruction: every block freed once
        Fake::reset();
        Buf a, b;
        CHECK(a.reserve(8, 8) == 0 && b.reserve(9, 9) == 0);
        uint8_t *pa = a, *pb = b;
        Buf c(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && c.p == pa && c.cap == 8 && Fake::frees == 0);
        c = std::move(b);   // c's block goes, b's moves in
        CHECK(Fake::frees == 1 && c.p == pb && c.cap == 9 && b.p == nullptr && b.cap == 0);
        Buf &self = c;
        c = std::move(self);
        CHECK(c.p == pb && Fake::frees == 1);
        c.release();
        c.release();
        CHECK(Fake::frees == 2 && c.p == nullptr && c.cap == 0 && Fake::live == 0);
        CHECK(a.reserve(4, 4) == 0);   // a moved-from owner is an empty one
        Three t, u;
        CHECK(t.reserve(100, 10) == 0);
        u = std::move(t);   // a struct of owners moves member by member
        CHECK(u.kept(100, 10) && !t.kept(100, 10) && Fake::live == 4);
    }
    CHECK(Fake::live == 0 && Fake::frees == Fake::allocs);
    {   // 5. a stage whose third allocation fails says so, and does not pass for reserved afterwards
        Fake::reset(3);
        Three t;
        CHECK(t.reserve(1000, 50) == kNoMemory);
        CHECK(t.a.p && t.b.p && !t.c.p && t.c.cap == 0);
        CHECK(!t.kept(1000, 50));                    // a size recorded before the allocations would say yes here
        CHECK(t.reserve(1000, 50) == 0 && t.kept(1000, 50) && t.c.p && Fake::live == 3);
        CHECK(t.reserve(900, 50) == 0 && Fake::allocs == 6);   // serves a smaller call as it is
        CHECK(!t.kept(1000, 51) && !t.kept(1001, 50));
    }
    CHECK(Fake::live == 0 && Fake::frees + 1 == Fake::allocs);   // the failed allocation has no free
    {   // 6. the scratch owner's rule (pcabi_scratch.h): counts in elements; nothing when they fit, else
        //    the old block goes first and max(count elements, 64 KiB) come -- one allocation per growth
        //    (the real policy bumps the scratch generation once per allocation)
        Fake::reset(4);
        ScratchOf<Fake, int32_t> s;
        CHECK(s.ensure(0) == 0 && s.p == nullptr && Fake::allocs == 0);
        CHECK(s.ensure(10) == 0 && s.cap == 16384 && Fake::allocs == 1);             // 64 KiB of int32
        int32_t *p = s;
        p[16383] = 7;
        CHECK(s.ensure(16384) == 0 && s.ensure(1) == 0 && s.p == p && Fake::allocs == 1 && Fake::frees == 0);
        CHECK(s.ensure(16385) == 0 && s.cap == 16385 && Fake::allocs == 2 && Fake::frees == 1 && Fake::peak == 1);
        s[16384] = 8;
        CHECK(s.ensure(40000) == 0 && s.cap == 40000 && Fake::allocs == 3 && Fake::frees == 2 && Fake::peak == 1);
        CHECK(s.ensure(50000) == kNoMemory && s.p == nullptr && s.cap == 0 && Fake::live == 0 && Fake::frees == 3);
        CHECK(s.ensure(5) == 0 && s.p != nullptr && s.cap == 16384 && Fake::allocs == 5);   // the next call allocates
        ScratchOf<Fake> b;                                                           // bytes by default
        CHECK(b.ensure(1) == 0 && b.cap == 65536 && b.ensure(65537) == 0 && b.cap == 65537);
        b[65536] = 1;
        // PCABI_MIDDLE_INIT_CAPS: two to four fields, 0 (or a missing field) keeps the default
        using pcabi_internal::parse_middle_init_caps;
        auto caps = [](const char *e, int64_t raw, int64_t task, int64_t slots, int64_t arena) {
            const pcabi_internal::MiddleInitCaps c = parse_middle_init_caps(e);
            return c.raw == raw && c.task == task && c.slots == slots && c.arena == arena;
        };
        CHECK(caps(nullptr, 0, 0, 0, 0) && caps("", 0, 0, 0, 0) && caps("x", 0, 0, 0, 0));
        CHECK(caps("256,0,0", 256, 0, 0, 0) && caps("0,64,0", 0, 64, 0, 0) && caps("0,0,128", 0, 0, 128, 0));
        CHECK(caps("256,64,128", 256, 64, 128, 0) && caps("0,0,0,4096", 0, 0, 0, 4096) && caps("7,9", 7, 9, 0, 0));
        CHECK(caps("-1,-2,-3,-4", 0, 0, 0, 0) && caps("5", 5, 0, 0, 0));
    }
    CHECK(Fake::live == 0);
    // the copy and the clock the stages share
    std::vector<uint8_t> src(33u << 20), dst(src.size());
    for (size_t i = 0; i < src.size(); i += 4093) src[i] = (uint8_t)(i * 31);
    const double t0 = pcabi_internal::now_s();
    pcabi_internal::par_memcpy(dst.data(), src.data(), src.size());
    pcabi_internal::par_memcpy(dst.data(), src.data(), 5);
    CHECK(dst == src && pcabi_internal::now_s() >= t0);
    std::printf("hostdev ok\n");
    return 0;
}
