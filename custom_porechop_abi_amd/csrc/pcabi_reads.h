// pcabi_reads.h -- what the reader (pcabi_io.cpp) and the writers (pcabi_write.cpp) share: a batch of
// reads, the vector its large buffers live in, and the io threads. Declarations; pcabi_io.cpp implements.
#pragma once

#include "pcabi_hostdev.h"

namespace pcabi_internal {
// Large batch buffers come from a process-wide cache of huge-page mappings (pcabi_io.cpp bigmem).
namespace bigmem {
void *get(size_t bytes);
void put(void *p, size_t bytes);
}  // namespace bigmem
}  // namespace pcabi_internal

// vector whose resize() leaves new elements uninitialised (the batch buffers are written once,
// in parallel; zero-filling gigabytes first would cost as much as the parse)
template <typename T>
struct NoInit : std::allocator<T> {
    template <typename U>
    struct rebind { using other = NoInit<U>; };
    NoInit() = default;
    template <typename U>
    NoInit(const NoInit<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(pcabi_internal::bigmem::get(n * sizeof(T))); }
    void deallocate(T *p, size_t n) noexcept { pcabi_internal::bigmem::put(p, n * sizeof(T)); }
    template <typename U>
    void construct(U *p) noexcept { ::new ((void *)p) U; }
    template <typename U, typename... A>
    void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};
template <typename T, typename U>
bool operator==(const NoInit<T> &, const NoInit<U> &) { return true; }
template <typename T, typename U>
bool operator!=(const NoInit<T> &, const NoInit<U> &) { return false; }
template <typename T>
using RawVec = std::vector<T, NoInit<T>>;

struct pcabi_reads {
    int type = -1;
    int64_t n = 0;
    RawVec<char> names;                      // full headers (after '@' / '>'), back to back
    std::vector<int64_t> name_off{0};
    RawVec<char> seq;                        // upper-cased, U->T for RNA reads
    std::vector<int64_t> seq_off{0};
    RawVec<char> qual;                       // padded with '+' to the sequence length
    std::vector<int64_t> qual_off{0};
    std::vector<uint8_t> rna;
    RawVec<char> spacer;                     // FASTQ '+' lines (stripped)
    std::vector<int64_t> spacer_off{0};
    RawVec<uint8_t> codes;                   // Dna5, 4-aligned starts, 16 B tail padding (N)
    std::vector<int64_t> code_off;
    std::vector<int32_t> len;
    // a BAM reader with pcabi_fastx_keep_aux: the records' aux bytes and whether their bases are as stored;
    // empty otherwise (aux_off too)
    std::vector<uint8_t> aux, as_stored;
    std::vector<int64_t> aux_off;
    // a FASTA / FASTQ reader with pcabi_fastx_header_tags: the aux bytes were parsed from the headers, which
    // still hold them as text behind their first tab
    bool tags_from_headers = false;
};

inline int io_threads() { return pcabi_internal::io_thread_count(); }   // PCABI_IO_THREADS, default min(cores, 16)

// fn(t) for t in [0, threads), each on a thread of its own (inline for one): a range of the work by
// index, or items taken from a shared counter
template <class F>
void fan_out(int threads, F &&fn) {
    if (threads <= 1) {
        fn(0);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t) th.emplace_back(fn, t);
    for (auto &x : th) x.join();
}
