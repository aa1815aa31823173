// pcabi_scratch.h -- the owner of the host-buffer engines', the middle scan's and the seeds' device
// scratch (pcabi_hostapi.hip, pcabi_middle.hip, pcabi_seed.hip), built on Owned<Mem, T> (pcabi_hostdev.h), and
// the one reader of PCABI_MIDDLE_INIT_CAPS. What names a HIP type sits under __HIPCC__; the growth
// rule compiles with a plain C++ compiler (tests/hostdev_main.cpp runs it over a fake allocator).
#pragma once

#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "pcabi_hostdev.h"

// Bumped by every device (re)allocation of the engine's and the seeds' scratch and by every new
// seed plan: a captured round graph (pcabi_middle.hip run_round) holds their addresses and launch
// arguments, and is replayed only while the generation it was captured at holds.
extern std::atomic<uint64_t> g_buf_gen;

// Debug switch PCABI_POISON (pcabi_engine.hip): every fresh scratch allocation and every growth is
// filled with one byte before use; < 0 when off.
int pcabi_poison_byte();
void pcabi_poison(void *p, size_t bytes);

namespace pcabi_internal {

// Scratch of T that grows on demand and keeps nothing across a growth: ensure(count) does nothing
// when count elements fit, else the old block goes first and max(count elements, 64 KiB) are
// allocated. A failure leaves {nullptr, 0}, so the next call allocates again.
template <class Mem, class T = uint8_t>
struct ScratchOf : Owned<Mem, T> {
    int ensure(int64_t count) {
        constexpr int64_t kMin = (int64_t)(((size_t)1 << 16) + sizeof(T) - 1) / (int64_t)sizeof(T);
        return this->reserve(count, std::max(count, kMin));
    }
};

// PCABI_MIDDLE_INIT_CAPS="raw,task[,slots[,arena]]" (tests: first capacities small enough to overflow
// and grow): the seeds' raw-hit slabs and band task regions, the queued rounds' candidate-DP task
// slots, the shadow arena's bytes. A field that is missing, 0 or negative keeps its default (0 here).
struct MiddleInitCaps {
    int64_t raw = 0, task = 0, slots = 0, arena = 0;
};
inline MiddleInitCaps parse_middle_init_caps(const char *e) {
    MiddleInitCaps c;
    long long v[4] = {0, 0, 0, 0};
    const int got = e ? std::sscanf(e, "%lld,%lld,%lld,%lld", &v[0], &v[1], &v[2], &v[3]) : 0;
    int64_t *f[4] = {&c.raw, &c.task, &c.slots, &c.arena};
    for (int k = 0; k < 4; ++k)
        if (k < got && v[k] > 0) *f[k] = v[k];
    return c;
}
inline MiddleInitCaps middle_init_caps() { return parse_middle_init_caps(std::getenv("PCABI_MIDDLE_INIT_CAPS")); }

#ifdef __HIPCC__
// hipMalloc / hipFree with the scratch generation bumped and the poison applied on every allocation
struct ScratchAlloc {
    static int alloc(void **p, size_t n) {
        g_buf_gen.fetch_add(1);
        const hipError_t e = hipMalloc(p, n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            return fail(PCABI_E_NOMEM, "hipMalloc failed (" + std::to_string(n) + " bytes): " + hipGetErrorString(e));
        }
        pcabi_poison(*p, n);
        return 0;
    }
    static void free(void *p) { (void)hipFree(p); }
};
template <class T = uint8_t>
using Scratch = ScratchOf<ScratchAlloc, T>;
#endif

}  // namespace pcabi_internal
