// pcabi_io.cpp -- native FASTA / FASTQ (plain or gzip) and unaligned BAM reader for the
// adapter-alignment engine (host code, part of libpcabi.so; declared in include/pcabi.h). The writers of
// the batches it makes are csrc/pcabi_write.cpp; csrc/pcabi_reads.h holds what the two share.
//
// The reader turns a sequence file straight into the engine's input layout -- Dna5 codes packed
// back to back at 4-aligned offsets with 16 bytes of tail padding (engine.SeqPack) -- plus the
// read names, upper-cased sequence text and qualities, in batches, with the reference's parsing
// rules:
//   * file type from the first decoded character: '>' FASTA, '@' FASTQ, else an error
//     (porechop_abi/misc.py:84-105); gzip by its magic bytes, bzip2 / zip refused (:60-81); a file
//     whose first decoded bytes are "BAM" is an unaligned BAM file: its records (pcabi_bam.h) become
//     a FASTQ batch, unpacked on the device when the reader inflates there (BamState below);
//   * FASTQ: 4 lines per record, each stripped; name = line[1:] (the full header), sequence,
//     spacer, qualities (misc.py:148-165); a blank or truncated record is a parse error (the
//     reference dies on it too);
//   * FASTA: stripped lines, blank lines skipped, '>' starts a record whose sequence is the
//     concatenation of the following lines; a record with an empty name is not emitted and its
//     sequence carries over (misc.py:123-145, replicated exactly);
//   * lines end at \n, \r\n or \r (Python's universal newlines), strip() removes the ASCII
//     characters str.isspace() accepts;
//   * NanoporeRead's normalisation (porechop_abi/nanopore_read.py:31-44): sequence upper-cased,
//     U -> T when the read has more U than T (rna flag), qualities padded with '+' to the
//     sequence length.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cctype>
#include <cerrno>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <unordered_map>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_bam.h"
#include "pcabi_hostdev.h"
#include "pcabi_reads.h"

using pcabi_internal::fail;
using pcabi_internal::now_s;

namespace {

inline bool py_space(unsigned char c) {   // str.isspace() on ASCII
    return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20);
}

uint8_t g_dna5[256];
const bool g_dna5_init = [] {
    for (int i = 0; i < 256; ++i) g_dna5[i] = 4;
    const char *s = "ACGTU", *l = "acgtu";
    const uint8_t v[5] = {0, 1, 2, 3, 3};
    for (int k = 0; k < 5; ++k) {
        g_dna5[(unsigned char)s[k]] = v[k];
        g_dna5[(unsigned char)l[k]] = v[k];
    }
    return true;
}();

}  // namespace

// A BAM input's state. win[0, end) is a window of the inflated bytes (on the device path mirrored there,
// pcabi_bam.hip BamDev): the record chain is walked from `at`, whole records are unpacked into the
// stage -- a table, their names and their sequence / quality / code bytes in the batch layout, whose
// code offsets are multiples of four, so any run of staged records is appended to a batch by plain
// copies -- and the incomplete record at the window's end is carried in front of the next bytes.
struct BamState {
    std::vector<uint8_t> win;
    size_t at = 0, end = 0;
    int64_t base = 0;                 // the stream offset of win[0] (error messages)
    int64_t total_est = 0;            // the stream's inflated length (the index's sum), or a guess from the file size
    bool header_done = false, eof = false;
    int pending = 0;                  // a fault: raised once the records before it are delivered
    std::string pending_msg;
    std::vector<pcabi_bam_rec> recs;  // the stage; [next, size) not yet delivered
    size_t next = 0;
    std::vector<char> names;
    std::vector<int64_t> name_off;
    std::vector<uint8_t> h_seq, h_qual, h_codes;   // the host path's outputs
    const uint8_t *seq = nullptr, *qual = nullptr, *codes = nullptr;
    pcabi_internal::BamDev *dev = nullptr;
    std::string header_text;          // the input's header text (pcabi_fastx_bam_header)
    bool keep_aux = false;            // pcabi_fastx_keep_aux: the staged records' aux bytes, copied from the window
    std::vector<uint8_t> aux, stored;
    std::vector<int64_t> aux_off;
};

struct pcabi_fastx {
    gzFile f = nullptr;
    pcabi_internal::GunzipReader *dev = nullptr;   // block-gzipped input inflated on the device, instead of f
    pcabi_internal::GzStreamReader *zs = nullptr;  // gzip without an index inflated on the device, instead of f
    void *zmap = nullptr;                          // the compressed bytes of dev / zs, mapped whole
    size_t zmap_len = 0;
    int type = -1;                 // PCABI_FASTA / PCABI_FASTQ
    BamState *bam = nullptr;       // the input is a BAM file (type PCABI_FASTQ): records instead of lines
    std::vector<char> buf;         // gzip: decoded bytes [0, end)
    const char *base = nullptr;    // buf.data(), or the mapping of a plain file
    void *map = nullptr;           // plain files are memory-mapped whole
    size_t map_len = 0;
    size_t pin = (size_t)-1;       // refills keep the bytes from here on (a batch's records)
    size_t pos = 0, end = 0;
    bool eof = false;
    bool err = false;              // a read error (e.g. a truncated gzip stream): the next call fails
    int64_t line_no = 0;
    bool raw = false;              // keep the file's text (misc.load_fasta_or_fastq tuples)
    size_t size_hint = 0;          // decoded bytes expected (file size; x4 for gzip)
    size_t released = 0;           // mapped file bytes before this have had their page mappings dropped
    // populate-ahead (plain files): a helper thread maps the pages up to kAhead bytes past the
    // reader's published position, so the record scan finds them mapped (r05: the scan's own
    // faults were half a 200 MB batch's read time)
    std::thread ahead;
    std::atomic<bool> ahead_stop{false};
    std::atomic<size_t> reader_at{0};
    ~pcabi_fastx() {
        ahead_stop = true;
        if (ahead.joinable()) ahead.join();
    }
    // FASTA state that crosses batch boundaries
    bool fa_have_name = false;     // a header was seen (its name may be empty)
    std::string fa_name, fa_seq;
    int txt_named = -1;            // pcabi_fastx_next_text: the last header had a name (1), none (0), no header (-1)
    // pcabi_fastx_header_tags: every batch's aux bytes are parsed from its headers, on tags_device (< 0: the host build)
    bool header_tags = false;
    int tags_device = -1;
    pcabi_internal::AuxParseDev *tags_dev = nullptr;
};

// Large batch buffers (>= 8 MB, r05) come from anonymous mappings with transparent huge pages and
// go back to a small process-wide cache when a batch is freed, so the next batch reuses pages
// that are already faulted in: first-touch faults and the unmapping of gigabyte buffers cost
// about as much as the parse itself (4 KB pages: ~400 k faults per 1.6 GB batch).
namespace pcabi_internal {
namespace bigmem {
namespace {
constexpr size_t kBig = 8ull << 20;   // r05: 64 MB left the buffers of 6 k-read batches to malloc, which
                                      // maps and unmaps them per batch (e2e 3.5x slower at that size)
// Free blocks kept for reuse: PCABI_IO_CACHE_MB, default min(4 GB, physical memory / 8) -- enough
// for the batches a pipeline keeps in flight; pcabi_io_release_cache() returns them all.
size_t cache_max() {
    static const size_t v = [] {
        const char *e = std::getenv("PCABI_IO_CACHE_MB");
        if (e && e[0]) return (size_t)std::max(0LL, std::atoll(e)) << 20;
        const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGE_SIZE);
        const size_t ram = (pages > 0 && psz > 0) ? (size_t)pages * (size_t)psz : (8ull << 30);
        return std::min<size_t>(4ull << 30, ram / 8);
    }();
    return v;
}
std::mutex mu;
std::unordered_map<void *, size_t> mapped;          // live and cached blocks -> mapped bytes
std::vector<std::pair<void *, size_t>> cache;       // free blocks
size_t cached = 0;

inline size_t round2m(size_t b) { return (b + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1); }
}  // namespace

void *get(size_t bytes) {
    if (bytes < kBig) return ::operator new(bytes);
    std::lock_guard<std::mutex> g(mu);
    size_t best = SIZE_MAX, bi = 0;
    for (size_t i = 0; i < cache.size(); ++i)
        if (cache[i].second >= bytes && cache[i].second < best) { best = cache[i].second; bi = i; }
    if (best != SIZE_MAX && best <= 2 * bytes + (256ull << 20)) {
        void *p = cache[bi].first;
        cached -= best;
        cache.erase(cache.begin() + (long)bi);
        return p;
    }
    // 1/8 headroom: the next batch's buffers, sized exactly and a little larger or smaller than
    // these, still fit a cached block (already faulted in) instead of a fresh mapping
    const size_t m = round2m(bytes + bytes / 8);
    void *p = mmap(nullptr, m, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) throw std::bad_alloc();
#ifdef MADV_HUGEPAGE
    madvise(p, m, MADV_HUGEPAGE);
#endif
    mapped[p] = m;
    return p;
}

void put(void *p, size_t bytes) {
    if (!p) return;
    if (bytes < kBig) {
        ::operator delete(p);
        return;
    }
    std::lock_guard<std::mutex> g(mu);
    const size_t m = mapped.at(p);
    cache.emplace_back(p, m);
    cached += m;
    while (cached > cache_max() && !cache.empty()) {   // drop the oldest
        munmap(cache.front().first, cache.front().second);
        mapped.erase(cache.front().first);
        cached -= cache.front().second;
        cache.erase(cache.begin());
    }
}
void release() {
    std::lock_guard<std::mutex> g(mu);
    for (auto &c : cache) {
        munmap(c.first, c.second);
        mapped.erase(c.first);
    }
    cache.clear();
    cached = 0;
}
}  // namespace bigmem
}  // namespace pcabi_internal
namespace bigmem = pcabi_internal::bigmem;

extern "C" void pcabi_io_release_cache(void) { bigmem::release(); }

namespace {

// Next line (without its terminator) as [*p, *p + *n); false at end of file. Terminators are
// found with memchr: the first '\n', then any '\r' before it (CRLF, or a lone CR that ends the
// line earlier).
// The first '\n' or '\r' in [s, e), or nullptr: one pass over the line (r05; two memchr passes --
// '\n', then '\r' before it -- read every byte twice, the record scan's main cost once the pages are
// mapped ahead). AVX2 where the CPU has it.
#if defined(__x86_64__)
__attribute__((target("avx2"))) const char *find_eol_avx2(const char *s, const char *e) {
    const __m256i lf = _mm256_set1_epi8('\n'), cr = _mm256_set1_epi8('\r');
    for (; s + 32 <= e; s += 32) {
        const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s));
        const unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_or_si256(_mm256_cmpeq_epi8(v, lf), _mm256_cmpeq_epi8(v, cr)));
        if (m) return s + __builtin_ctz(m);
    }
    for (; s < e; ++s)
        if (*s == '\n' || *s == '\r') return s;
    return nullptr;
}
#endif
const char *find_eol(const char *s, const char *e) {
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return find_eol_avx2(s, e);
#endif
    const char *nl = (const char *)std::memchr(s, '\n', (size_t)(e - s));
    const char *cr = (const char *)std::memchr(s, '\r', (size_t)((nl ? nl : e) - s));
    return cr ? cr : nl;
}

bool next_line(pcabi_fastx *r, const char **p, size_t *n) {
    for (;;) {
        const char *base = r->base;
        const char *s0 = base + r->pos, *e0 = base + r->end;
        // the first line end of either kind: a '\r' before the first '\n' is the line's end
        const char *eol = find_eol(s0, e0);
        const char *nl = eol && *eol == '\n' ? eol : nullptr;
        const char *cr = eol && *eol == '\r' ? eol : nullptr;
        if (cr && (cr + 1 < e0 || r->eof)) {          // \r ends the line (a following \n is eaten)
            *p = s0;
            *n = (size_t)(cr - s0);
            r->pos = (size_t)(cr + 1 - base) + ((cr + 1 < e0 && cr[1] == '\n') ? 1 : 0);
            ++r->line_no;
            return true;
        }
        if (nl && !cr) {
            *p = s0;
            *n = (size_t)(nl - s0);
            r->pos = (size_t)(nl + 1 - base);
            ++r->line_no;
            return true;
        }
        if (r->eof) {
            if (r->pos < r->end) {   // last line without a terminator
                *p = s0;
                *n = r->end - r->pos;
                r->pos = r->end;
                ++r->line_no;
                return true;
            }
            return false;
        }
        // refill: keep the partial line (and a pinned batch), grow if it fills the buffer
        const size_t from = std::min(r->pos, r->pin);
        if (from > 0) {
            std::memmove(r->buf.data(), r->buf.data() + from, r->end - from);
            r->pos -= from;
            r->end -= from;
            if (r->pin != (size_t)-1) r->pin -= from;
        }
        if (r->buf.size() - r->end < (1u << 20)) r->buf.resize(std::max<size_t>(r->buf.size() * 2, 4u << 20));
        r->base = r->buf.data();
        const size_t room = std::min<size_t>(r->buf.size() - r->end, 1u << 30);
        int got;
        const char *zmsg = nullptr;
        bool bad;
        if (r->dev) {
            const int64_t k = pcabi_internal::gunzip_reader_read(r->dev, r->buf.data() + r->end, (int64_t)room);
            got = k < 0 ? -1 : (int)k;
            bad = k < 0;
            if (bad) zmsg = pcabi_last_error();
        } else if (r->zs) {
            const int64_t k = pcabi_internal::gzstream_reader_read(r->zs, r->buf.data() + r->end, (int64_t)room);
            got = k < 0 ? -1 : (int)k;
            bad = k < 0;
            if (bad) zmsg = pcabi_last_error();
        } else {
            got = gzread(r->f, r->buf.data() + r->end, (unsigned)room);
            int zerr = Z_OK;
            zmsg = got < 0 || got == 0 ? gzerror(r->f, &zerr) : nullptr;
            bad = got < 0 || (got == 0 && zerr != Z_OK && zerr != Z_STREAM_END);
        }
        if (bad) {
            // a damaged or truncated gzip stream: the reference's gzip module raises too
            // (EOFError "Compressed file ended before the end-of-stream marker was reached")
            const std::string msg = std::string("read error: ") + (zmsg ? zmsg : "?");
            fail(PCABI_E_PARSE, msg);
            r->err = true;
            r->eof = true;
            r->end = r->pos;   // drop the partial data
            return false;
        }
        if (got == 0) r->eof = true;
        r->end += (size_t)got;
    }
}

void strip(const char **p, size_t *n) {
    const char *a = *p;
    size_t m = *n;
    while (m && py_space((unsigned char)a[0])) { ++a; --m; }
    while (m && py_space((unsigned char)a[m - 1])) --m;
    *p = a;
    *n = m;
}

uint8_t g_upper[256];
const bool g_upper_init = [] {
    for (int i = 0; i < 256; ++i) g_upper[i] = (uint8_t)((i >= 'a' && i <= 'z') ? i - 32 : i);
    return true;
}();

// A record is appended in pieces (name, sequence, qualities) straight from the line buffer.
void add_name(pcabi_reads *b, const char *name, size_t nn) {
    b->names.insert(b->names.end(), name, name + nn);
    b->name_off.push_back((int64_t)b->names.size());
}

// Sequence with NanoporeRead's normalisation unless raw: upper case, U -> T when the read holds
// more U than T; Dna5 codes (U and T are both code 3) into the engine layout in the same pass.
void add_seq(pcabi_reads *b, const char *seq, size_t ns, bool raw) {
    const size_t s0 = b->seq.size();
    b->seq.resize(s0 + ns);
    char *d = b->seq.data() + s0;
    const int64_t off = (int64_t)b->codes.size();
    const size_t padded = (ns + 3) & ~(size_t)3;
    b->codes.resize((size_t)off + padded);
    uint8_t *c = b->codes.data() + off;
    int64_t nu = 0, nt = 0;
    if (raw) {
        std::memcpy(d, seq, ns);
        for (size_t i = 0; i < ns; ++i) c[i] = g_dna5[(unsigned char)seq[i]];
    } else {
        for (size_t i = 0; i < ns; ++i) {
            const uint8_t u = g_upper[(unsigned char)seq[i]];
            nu += (u == 'U');
            nt += (u == 'T');
            d[i] = (char)u;
            c[i] = g_dna5[u];
        }
    }
    for (size_t i = ns; i < padded; ++i) c[i] = 4;
    const bool rna = !raw && nu > nt;
    if (rna)
        for (size_t i = 0; i < ns; ++i)
            if (d[i] == 'U') d[i] = 'T';
    b->rna.push_back(rna ? 1 : 0);
    b->seq_off.push_back((int64_t)b->seq.size());
    b->code_off.push_back(off);
    b->len.push_back((int32_t)ns);
}

// Qualities padded with '+' to the sequence length unless raw; closes the record.
void add_qual(pcabi_reads *b, const char *q, size_t nq, size_t ns, bool raw, const char *sp = nullptr,
              size_t nsp = 0) {
    b->qual.insert(b->qual.end(), q, q + nq);
    if (!raw && nq < ns) b->qual.insert(b->qual.end(), ns - nq, '+');
    b->qual_off.push_back((int64_t)b->qual.size());
    b->spacer.insert(b->spacer.end(), sp, sp + nsp);
    b->spacer_off.push_back((int64_t)b->spacer.size());
    ++b->n;
}

void add_record(pcabi_reads *b, const char *name, size_t nn, const char *seq, size_t ns, const char *q, size_t nq,
                bool raw = false) {
    add_name(b, name, nn);
    add_seq(b, seq, ns, raw);
    add_qual(b, q, nq, ns, raw);
}

void finish_batch(pcabi_reads *b) { b->codes.resize(b->codes.size() + 16, 4); }

// A FASTQ record as spans of the batch's text (offsets from the batch start).
struct Span {
    size_t no, nn, so, sn, xo, xn, qo, qn;
};

#ifndef MADV_POPULATE_READ
#define MADV_POPULATE_READ 22
#endif
// The populate-ahead loop of a mapped file (pcabi_fastx::ahead): [at, end) in 8 MB steps, never more
// than kAhead bytes past the reader. MADV_POPULATE_READ (Linux >= 5.14) maps a step in one call;
// where it is refused the helper touches one byte per page instead (the faults then land here).
void populate_ahead(pcabi_fastx *r, size_t at, size_t end) {
    constexpr size_t kStep = 8u << 20, kAhead = 512u << 20;
    bool populate = true;
    volatile unsigned sink = 0;
    const char *m = (const char *)r->map;
    while (!r->ahead_stop.load(std::memory_order_relaxed) && at < end) {
        const size_t rd = r->reader_at.load(std::memory_order_relaxed);
        at = std::max(at, rd & ~(size_t)4095);        // never behind the reader (its pages are mapped)
        if (at >= end) break;
        const size_t lim = rd + kAhead;
        if (at >= lim) {
            std::this_thread::sleep_for(std::chrono::microseconds(200));
            continue;
        }
        const size_t n = std::min({kStep, end - at, lim - at});
        if (!populate || madvise((void *)(m + at), n, MADV_POPULATE_READ) != 0) {
            populate = false;
            unsigned x = 0;
            for (size_t q = at; q < at + n; q += 4096) x += (unsigned char)m[q];
            sink = sink + x;
        }
        at += n;
    }
}

}  // namespace

int pcabi_internal::io_thread_count() {
    if (const char *e = std::getenv("PCABI_IO_THREADS")) {
        const int t = std::atoi(e);
        if (t > 0) return std::min(t, 256);
    }
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hw ? hw : 1u, 16u));
}

namespace {

// The records of one FASTQ batch, normalised into b in parallel: offsets first (prefix sums),
// then every thread fills a contiguous range of records (names, sequence + Dna5 codes + rna
// flag, qualities + padding, spacer lines).
void fill_fastq(pcabi_reads *b, const char *T, const std::vector<Span> &rec, bool raw) {
    const size_t n = rec.size();
    const size_t n0 = (size_t)b->n;
    b->name_off.resize(n0 + n + 1);
    b->seq_off.resize(n0 + n + 1);
    b->qual_off.resize(n0 + n + 1);
    b->spacer_off.resize(n0 + n + 1);
    b->code_off.resize(n0 + n);
    b->len.resize(n0 + n);
    b->rna.resize(n0 + n);
    int64_t code_end = (int64_t)b->codes.size();
    for (size_t i = 0; i < n; ++i) {
        const Span &r = rec[i];
        b->name_off[n0 + i + 1] = b->name_off[n0 + i] + (int64_t)r.nn;
        b->seq_off[n0 + i + 1] = b->seq_off[n0 + i] + (int64_t)r.sn;
        b->qual_off[n0 + i + 1] = b->qual_off[n0 + i] + (int64_t)(raw ? r.qn : std::max(r.qn, r.sn));
        b->spacer_off[n0 + i + 1] = b->spacer_off[n0 + i] + (int64_t)r.xn;
        b->code_off[n0 + i] = code_end;
        b->len[n0 + i] = (int32_t)r.sn;
        code_end += (int64_t)((r.sn + 3) & ~(size_t)3);
    }
    // exact sizes, known from the record scan (finish_batch's 16 bytes of padding included): the
    // blocks of one batch then match the next batch's, and the block cache hands them back already
    // faulted in (a file-sized reservation per batch made every free an unmapping, r05)
    b->names.reserve((size_t)b->name_off[n0 + n]);
    b->seq.reserve((size_t)b->seq_off[n0 + n]);
    b->qual.reserve((size_t)b->qual_off[n0 + n]);
    b->codes.reserve((size_t)code_end + 16);
    b->names.resize((size_t)b->name_off[n0 + n]);
    b->seq.resize((size_t)b->seq_off[n0 + n]);
    b->qual.resize((size_t)b->qual_off[n0 + n]);
    b->spacer.resize((size_t)b->spacer_off[n0 + n]);
    b->codes.resize((size_t)code_end);
    auto work = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const Span &r = rec[i];
            const size_t k = n0 + i;
            std::memcpy(b->names.data() + b->name_off[k], T + r.no, r.nn);
            std::memcpy(b->spacer.data() + b->spacer_off[k], T + r.xo, r.xn);
            char *d = b->seq.data() + b->seq_off[k];
            uint8_t *c = b->codes.data() + b->code_off[k];
            const unsigned char *sq = (const unsigned char *)T + r.so;
            int64_t nu = 0, nt = 0;
            if (raw) {
                std::memcpy(d, sq, r.sn);
                for (size_t j = 0; j < r.sn; ++j) c[j] = g_dna5[sq[j]];
            } else {
                for (size_t j = 0; j < r.sn; ++j) {
                    const uint8_t u = g_upper[sq[j]];
                    nu += (u == 'U');
                    nt += (u == 'T');
                    d[j] = (char)u;
                    c[j] = g_dna5[u];
                }
            }
            for (size_t j = r.sn; j < ((r.sn + 3) & ~(size_t)3); ++j) c[j] = 4;
            const bool rna = !raw && nu > nt;
            if (rna)
                for (size_t j = 0; j < r.sn; ++j)
                    if (d[j] == 'U') d[j] = 'T';
            b->rna[k] = rna ? 1 : 0;
            char *q = b->qual.data() + b->qual_off[k];
            std::memcpy(q, T + r.qo, r.qn);
            if (!raw && r.qn < r.sn) std::memset(q + r.qn, '+', r.sn - r.qn);
        }
    };
    const int nt = (int)std::min<size_t>((size_t)io_threads(), std::max<size_t>(1, n / 256));
    fan_out(nt, [&](int t) { work(n * t / nt, n * (t + 1) / nt); });
    b->n = (int64_t)(n0 + n);
}

}  // namespace

extern "C" {

static int fastx_open_impl(const char *path, int raw, int device, int flags, pcabi_fastx **out) {
    if (!path || !out) return fail(PCABI_E_ARG, "bad arguments");
    *out = nullptr;
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return fail(PCABI_E_ARG, std::string("could not find ") + path);
    unsigned char magic[4] = {0, 0, 0, 0};
    const size_t nm = std::fread(magic, 1, 4, fp);
    std::fclose(fp);
    if (nm >= 3 && magic[0] == 0x42 && magic[1] == 0x5a && magic[2] == 0x68)
        return fail(PCABI_E_ARG, "cannot use bzip2 format - use gzip instead");
    if (nm >= 4 && magic[0] == 0x50 && magic[1] == 0x4b && magic[2] == 0x03 && magic[3] == 0x04)
        return fail(PCABI_E_ARG, "cannot use zip format - use gzip instead");
    const bool gz = nm >= 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    pcabi_fastx *r = new pcabi_fastx();
    r->raw = raw != 0;
    if (!gz) {
        // plain text: map the file, lines are read in place (no copies, no refills)
        const int fd = ::open(path, O_RDONLY);
        struct stat st;
        if (fd >= 0 && fstat(fd, &st) == 0 && st.st_size > 0) {
            // mapped lazily (r05): the record scan faults its batch in as it goes (fault-around maps
            // 16 pages a fault); MAP_POPULATE mapped the whole file before the first batch could be
            // parsed (~80 ms of a 1.6 GB file's first batch, nothing else overlapping it)
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
                r->map = m;
                r->map_len = (size_t)st.st_size;
                r->base = (const char *)m;
                r->end = r->map_len;
                r->eof = true;
            }
        }
        if (fd >= 0) ::close(fd);
    }
    if (gz && device >= 0) {
        // block-gzipped (every member lists its size): map the compressed file, index it, inflate
        // group by group on the device. Anything else falls through to zlib.
        const int fd = ::open(path, O_RDONLY);
        struct stat st;
        if (fd >= 0 && fstat(fd, &st) == 0 && st.st_size > 0) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                const int rc = pcabi_internal::gunzip_reader_open((const uint8_t *)m, (int64_t)st.st_size, device, &r->dev);
                if (rc < 0 || !r->dev) munmap(m, (size_t)st.st_size);
                if (rc < 0) {
                    ::close(fd);
                    delete r;
                    return rc;
                }
                if (r->dev) {
                    r->zmap = m;
                    r->zmap_len = (size_t)st.st_size;
                }
            }
        }
        if (fd >= 0) ::close(fd);
    }
    if (gz && device >= 0 && !r->dev && (flags & PCABI_OPEN_GUNZIP_PLAIN)) {
        // gzip without an index: map the compressed file, inflate span by span on the device
        const int fd = ::open(path, O_RDONLY);
        struct stat st;
        if (fd >= 0 && fstat(fd, &st) == 0 && st.st_size > 0) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                if (pcabi_internal::gzstream_reader_open((const uint8_t *)m, (int64_t)st.st_size, device, &r->zs) == 0 && r->zs) {
                    r->zmap = m;
                    r->zmap_len = (size_t)st.st_size;
                } else {
                    munmap(m, (size_t)st.st_size);
                }
            }
        }
        if (fd >= 0) ::close(fd);
    }
    if (!r->map && !r->dev && !r->zs) {
        gzFile f = gzopen(path, "rb");
        if (!f) {
            delete r;
            return fail(PCABI_E_ARG, std::string("could not open ") + path);
        }
        gzbuffer(f, 1u << 20);
        r->f = f;
    }
    if (FILE *sf = std::fopen(path, "rb")) {
        std::fseek(sf, 0, SEEK_END);
        const long sz = std::ftell(sf);
        std::fclose(sf);
        if (sz > 0) r->size_hint = (size_t)sz * ((magic[0] == 0x1f && magic[1] == 0x8b) ? 4 : 1);
    }
    if (!r->map) {
        r->buf.resize(4u << 20);
        r->base = r->buf.data();
        // type from the first decoded character
        while (r->end == 0 && !r->eof) {
            const int64_t got = r->dev  ? pcabi_internal::gunzip_reader_read(r->dev, r->buf.data(), (int64_t)r->buf.size())
                                : r->zs ? pcabi_internal::gzstream_reader_read(r->zs, r->buf.data(), (int64_t)r->buf.size())
                                        : (int64_t)gzread(r->f, r->buf.data(), (unsigned)r->buf.size());
            if (got < 0 && r->zs && r->end == 0) {
                // nothing decodes: the zlib reader finds no type either ("neither FASTA or FASTQ")
                r->eof = true;
                break;
            }
            if (got < 0 && r->dev) {   // a member that does not inflate, or a device error: not "no type"
                pcabi_fastx_close(r);
                return (int)got;
            }
            if (got <= 0) r->eof = true;
            else r->end = (size_t)got;
        }
    }
    const char c0 = r->end ? r->base[0] : 0;
    if (r->zs && r->end >= 4 && std::memcmp(r->base, "BAM", 3) == 0) {
        // a BAM file that is not block-gzipped: its records are read through zlib
        pcabi_fastx_close(r);
        return fastx_open_impl(path, raw, device, flags & ~PCABI_OPEN_GUNZIP_PLAIN, out);
    }
    if (!r->map && r->end >= 4 && std::memcmp(r->base, "BAM", 3) == 0) {
        // unaligned BAM: the version byte is checked with the header (a read error of the first batch)
        r->type = PCABI_FASTQ;
        r->bam = new BamState();
        r->bam->total_est = r->dev ? pcabi_internal::gunzip_reader_total(r->dev) : (int64_t)r->size_hint;
        if (r->dev) {
            pcabi_internal::gunzip_reader_unread(r->dev);   // the first group again, in place
            if (int rc = pcabi_internal::bam_dev_open(pcabi_internal::gunzip_reader_device(r->dev), &r->bam->dev)) {
                pcabi_fastx_close(r);
                return rc;
            }
        } else {
            r->bam->win.assign((const uint8_t *)r->base, (const uint8_t *)r->base + r->end);
            r->bam->end = r->end;
            r->bam->eof = r->eof;
        }
        r->pos = r->end = 0;
        std::vector<char>().swap(r->buf);
        r->base = nullptr;
    } else if (c0 == '>') r->type = PCABI_FASTA;
    else if (c0 == '@') r->type = PCABI_FASTQ;
    else {
        pcabi_fastx_close(r);
        return fail(PCABI_E_PARSE, std::string("File is neither FASTA or FASTQ: ") + path);
    }
    *out = r;
    return 0;
}

int pcabi_fastx_open(const char *path, int raw, pcabi_fastx **out) { return fastx_open_impl(path, raw, -1, 0, out); }

int pcabi_fastx_open_dev(const char *path, int raw, int device, pcabi_fastx **out) {
    return fastx_open_impl(path, raw, device, 0, out);
}

int pcabi_fastx_open_dev2(const char *path, int raw, int device, int flags, pcabi_fastx **out) {
    if (flags & ~PCABI_OPEN_GUNZIP_PLAIN) return fail(PCABI_E_ARG, "unknown open flags");
    return fastx_open_impl(path, raw, device, flags, out);
}

int pcabi_fastx_type(const pcabi_fastx *r) { return r ? r->type : -1; }

}  // extern "C"

namespace {
// Universal-newline line starts inside a memory-mapped file (the reader's line rules).
size_t line_after(const char *b, size_t n, size_t p) {
    while (p < n && b[p] != '\n' && b[p] != '\r') ++p;
    if (p < n && b[p] == '\r') {
        ++p;
        if (p < n && b[p] == '\n') ++p;
    } else if (p < n) {
        ++p;
    }
    return p;
}
size_t line_at_or_after(const char *b, size_t n, size_t p) {
    if (p == 0 || p >= n) return std::min(p, n);
    if (b[p - 1] == '\n' || (b[p - 1] == '\r' && b[p] != '\n')) return p;
    return line_after(b, n, p);
}
bool blank_after(const char *b, size_t n, size_t p) {   // only whitespace up to the line end
    for (; p < n && b[p] != '\n' && b[p] != '\r'; ++p)
        if (!std::isspace((unsigned char)b[p])) return false;
    return true;
}
// the nearest header ('>' at a line start) before position p, or n if none
size_t header_before(const char *b, size_t n, size_t p) {
    while (p > 0) {
        --p;
        if (b[p] == '>' && (p == 0 || b[p - 1] == '\n' || b[p - 1] == '\r')) return p;
    }
    return n;
}
}  // namespace

extern "C" {

int64_t pcabi_fastx_record_start(const pcabi_fastx *r, int64_t byte) {
    if (!r || !r->map) return fail(PCABI_E_ARG, "record starts need a plain (memory-mapped) file");
    const char *b = r->base;
    const size_t n = r->map_len;
    size_t p = line_at_or_after(b, n, byte < 0 ? 0 : (size_t)byte);
    for (; p < n; p = line_after(b, n, p)) {
        if (r->type == PCABI_FASTQ) {
            // a header line ('@') whose third line is the '+' line: a quality line may start
            // with '@', but two lines after it comes the next record's sequence, never '+'
            if (b[p] != '@') continue;
            const size_t q = line_after(b, n, line_after(b, n, p));
            if (q < n && b[q] == '+') return (int64_t)p;
        } else {
            // a header with a name, after a header with a name: an empty header's sequence runs
            // on into the next record (the reader's rule), so no record starts there
            if (b[p] != '>' || blank_after(b, n, p + 1)) continue;
            const size_t h = header_before(b, n, p);
            if (h == n || !blank_after(b, n, h + 1)) return (int64_t)p;
        }
    }
    return (int64_t)n;
}

int64_t pcabi_fastx_remaining(const pcabi_fastx *r) {
    if (!r || !r->map) return -1;
    return r->end > r->pos ? (int64_t)(r->end - r->pos) : 0;
}

int pcabi_fastx_set_range(pcabi_fastx *r, int64_t begin, int64_t end) {
    if (!r || !r->map) return fail(PCABI_E_ARG, "byte ranges need a plain (memory-mapped) file");
    if (begin < 0 || end < begin || (size_t)end > r->map_len) return fail(PCABI_E_ARG, "byte range outside the file");
    r->pos = (size_t)begin;
    r->end = (size_t)end;
    r->released = (size_t)begin & ~(size_t)4095;
    const size_t pg = (size_t)begin & ~(size_t)4095;
    if (end > begin) madvise((char *)r->map + pg, (size_t)end - pg, MADV_WILLNEED);
    r->eof = true;
    r->fa_have_name = false;
    r->fa_name.clear();
    r->fa_seq.clear();
    return 0;
}

void pcabi_fastx_close(pcabi_fastx *r) {
    if (!r) return;
    if (r->f) gzclose(r->f);
    if (r->bam) {
        pcabi_internal::bam_dev_close(r->bam->dev);   // before the streams it used go
        delete r->bam;
    }
    if (r->dev) pcabi_internal::gunzip_reader_close(r->dev);
    if (r->zs) pcabi_internal::gzstream_reader_close(r->zs);
    pcabi_internal::auxparse_dev_free(r->tags_dev);
    if (r->zmap) munmap(r->zmap, r->zmap_len);
    r->ahead_stop = true;                 // the populate-ahead helper leaves the mapping first
    if (r->ahead.joinable()) r->ahead.join();
    if (r->map) {
        // tearing down a gigabyte mapping takes ~0.1 s: off the caller's path
        void *m = r->map;
        const size_t n = r->map_len;
        std::thread([m, n] { munmap(m, n); }).detach();
    }
    delete r;
}

static int64_t bam_next(pcabi_fastx *r, int64_t max_reads, int64_t max_bases, pcabi_reads **out);

int64_t pcabi_fastx_next(pcabi_fastx *r, int64_t max_reads, int64_t max_bases, pcabi_reads **out) {
    if (!r || !out || max_reads <= 0) return fail(PCABI_E_ARG, "bad arguments");
    if (r->bam) return bam_next(r, max_reads, max_bases, out);
    if (r->map && !r->ahead.joinable() && r->end > r->pos + (64u << 20)) {
        // a large plain file read in batches: the helper maps pages ahead of the record scan
        r->reader_at.store(r->pos, std::memory_order_relaxed);
        r->ahead = std::thread(populate_ahead, r, r->pos & ~(size_t)4095, r->end);
    }
    pcabi_reads *b = new pcabi_reads();
    b->type = r->type;
    if (r->type != PCABI_FASTQ) {
        // FASTA appends record by record: sequence about the decoded bytes (FASTQ sizes its
        // buffers exactly from the record scan, fill_fastq)
        const size_t want = std::min<size_t>(r->size_hint / 2 + 4096, (size_t)std::min<int64_t>(max_bases, 1LL << 40));
        b->seq.reserve(want);
        b->codes.reserve(want + 4096);
    }
    int64_t bases = 0;
    const char *p;
    size_t n;
    // PCABI_IOPROF=1: per batch, the record scan's and the fill's milliseconds on stderr
    static const bool ioprof = [] {
        const char *e = std::getenv("PCABI_IOPROF");
        return e && e[0] == '1';
    }();
    const auto t_scan = std::chrono::steady_clock::now();
    if (r->type == PCABI_FASTQ) {
        std::vector<Span> rec;
        r->pin = r->pos;                 // the batch's bytes survive refills (shifted with the pin)
        auto rel = [&](const char *q) { return (size_t)(q - r->base) - r->pin; };
        while ((int64_t)rec.size() < max_reads && bases < max_bases) {
            if (!next_line(r, &p, &n)) break;
            strip(&p, &n);
            if (n == 0 || n == 1) {   // full_name.split()[0] fails in the reference (IndexError)
                delete b;
                r->pin = (size_t)-1;
                return fail(PCABI_E_PARSE, "could not be parsed - is it formatted correctly? (empty FASTQ header at line " +
                                               std::to_string(r->line_no) + ")");
            }
            Span sp{};
            sp.no = rel(p + 1);
            sp.nn = n - 1;
            const char *q;
            size_t qn;
            if (!next_line(r, &q, &qn)) { delete b; r->pin = (size_t)-1; return fail(PCABI_E_PARSE, "truncated FASTQ record"); }
            strip(&q, &qn);
            sp.so = rel(q);
            sp.sn = qn;
            if (!next_line(r, &q, &qn)) { delete b; r->pin = (size_t)-1; return fail(PCABI_E_PARSE, "truncated FASTQ record"); }
            if (r->raw) {
                strip(&q, &qn);
                sp.xo = rel(q);
                sp.xn = qn;
            }
            if (!next_line(r, &q, &qn)) { delete b; r->pin = (size_t)-1; return fail(PCABI_E_PARSE, "truncated FASTQ record"); }
            strip(&q, &qn);
            sp.qo = rel(q);
            sp.qn = qn;
            rec.push_back(sp);
            bases += (int64_t)sp.sn;
        }
        const auto t_fill = std::chrono::steady_clock::now();
        fill_fastq(b, r->base + r->pin, rec, r->raw);
        if (ioprof) {
            const auto t_end = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[pcabi io] batch %zu reads: scan %.2f ms, fill %.2f ms\n", rec.size(),
                         std::chrono::duration<double, std::milli>(t_fill - t_scan).count(),
                         std::chrono::duration<double, std::milli>(t_end - t_fill).count());
        }
        r->pin = (size_t)-1;
    } else {
        while (b->n < max_reads && bases < max_bases) {
            if (!next_line(r, &p, &n)) {
                if (r->fa_have_name && !r->fa_name.empty()) {
                    add_record(b, r->fa_name.data(), r->fa_name.size(), r->fa_seq.data(), r->fa_seq.size(), "", 0, r->raw);
                    bases += (int64_t)r->fa_seq.size();
                }
                r->fa_have_name = false;
                r->fa_name.clear();
                r->fa_seq.clear();
                break;
            }
            strip(&p, &n);
            if (n == 0) continue;
            if (p[0] == '>') {
                if (!r->fa_name.empty()) {
                    add_record(b, r->fa_name.data(), r->fa_name.size(), r->fa_seq.data(), r->fa_seq.size(), "", 0, r->raw);
                    bases += (int64_t)r->fa_seq.size();
                    r->fa_seq.clear();
                }
                r->fa_name.assign(p + 1, n - 1);
                r->fa_have_name = true;
            } else {
                r->fa_seq.append(p, n);
            }
        }
    }
    if (r->err) {
        delete b;
        return PCABI_E_PARSE;   // the message is pcabi_last_error()'s (next_line)
    }
    if (r->header_tags) {   // the headers' tags as aux bytes, where a BAM reader puts a record's
        if (const int rc = pcabi_internal::auxparse_headers(r->tags_device, r->tags_dev, (const uint8_t *)b->names.data(),
                                                            b->name_off.data(), b->n, &b->aux, &b->aux_off)) {
            delete b;
            return rc;
        }
        b->as_stored.assign((size_t)b->n, 1);
        b->tags_from_headers = true;
    }
    if (r->map) r->reader_at.store(r->pos, std::memory_order_relaxed);
    if (r->map) {
        // the batch holds copies of its records: the page mappings of the file bytes it consumed
        // are dropped as the reader goes (madvise takes the address space's lock shared), so the
        // final munmap has nothing left to tear down -- a whole-file teardown held the lock
        // exclusively for ~50 ms and stalled every other thread's page faults (r05 e2e timeline).
        // The bytes stay in the page cache; a later read of them faults them back in.
        const size_t upto = r->pos & ~(size_t)4095;
        if (upto >= r->released + (32u << 20)) {
            madvise((char *)r->map + r->released, upto - r->released, MADV_DONTNEED);
            r->released = upto;
        }
    }
    finish_batch(b);
    *out = b;
    return b->n;
}

// The next span of the decoded text holding whole records, cut where a reader starting afresh
// parses the same records as the continuous read: FASTQ after a record whose successor's line
// starts with '@'; FASTA before a header with a name whose preceding header had one (an empty
// header's sequence runs on into the next record). At least max_bytes unless the input ends first
// (one record may overshoot). *text stays valid until the next call on r. Returns 1, 0 at the end.
int pcabi_fastx_next_text(pcabi_fastx *r, int64_t max_bytes, const char **text, int64_t *len) {
    if (!r || !text || !len || max_bytes <= 0) return fail(PCABI_E_ARG, "bad arguments");
    if (r->bam) return fail(PCABI_E_ARG, "text spans are not available for a BAM input (its records are binary)");
    r->pin = r->pos;
    const char *p;
    size_t n;
    for (;;) {
        const size_t ls = r->pos - r->pin;           // this line's start, relative to the pin
        if (!next_line(r, &p, &n)) break;
        if (r->type == PCABI_FASTQ) {
            bool whole = true;
            for (int k = 0; k < 3 && whole; ++k) whole = next_line(r, &p, &n);
            if (!whole) break;                        // truncated: the chunk's reader reports it
            if ((int64_t)(r->pos - r->pin) >= max_bytes && r->pos < r->end && r->base[r->pos] == '@') break;
        } else {
            const char *q = p;
            size_t m = n;
            strip(&q, &m);
            if (m > 0 && q[0] == '>') {
                const int named = m > 1 ? 1 : 0;
                if ((int64_t)ls >= max_bytes && p[0] == '>' && named && r->txt_named == 1) {
                    r->pos = r->pin + ls;             // unread: the next span starts with this header
                    break;
                }
                r->txt_named = named;
            }
        }
    }
    *text = r->base + r->pin;
    *len = (int64_t)(r->pos - r->pin);
    r->pin = (size_t)-1;
    if (r->err) return PCABI_E_PARSE;
    return *len > 0 ? 1 : 0;
}

// ---- BAM records -----------------------------------------------------------------------------
// More inflated bytes behind the carried ones: > 0, 0 at the end of the stream (or at a read error, which
// becomes the pending fault), a negative code for a device error.
static int64_t bam_refill(pcabi_fastx *r) {
    BamState *s = r->bam;
    const size_t carry = s->end - s->at;
    const int64_t keep_from = (int64_t)s->at;
    if (s->at > 0) {
        std::memmove(s->win.data(), s->win.data() + s->at, carry);
        s->base += (int64_t)s->at;
        s->at = 0;
        s->end = carry;
    }
    int64_t got;
    std::string msg;
    if (r->dev) {
        const uint8_t *host = nullptr, *dev = nullptr;
        void *stream = nullptr;
        got = pcabi_internal::gunzip_reader_take(r->dev, &host, &dev, &stream);
        if (got < 0 && got != PCABI_E_PARSE) return got;
        if (got < 0) msg = pcabi_last_error();
        if (got > 0) {
            // (at the end of the stream nothing whole is left to unpack: the mirror may keep its old offsets)
            if (int rc = pcabi_internal::bam_dev_append(s->dev, keep_from, dev, got, stream)) return rc;
            if (s->win.size() < s->end + (size_t)got) s->win.resize(s->end + (size_t)got);
            std::memcpy(s->win.data() + s->end, host, (size_t)got);
        }
    } else {
        constexpr size_t kRead = 4u << 20;
        if (s->win.size() < s->end + kRead) s->win.resize(s->end + kRead);
        got = gzread(r->f, s->win.data() + s->end, (unsigned)kRead);
        int zerr = Z_OK;
        const char *zmsg = got <= 0 ? gzerror(r->f, &zerr) : nullptr;
        if (got < 0 || (got == 0 && zerr != Z_OK && zerr != Z_STREAM_END)) {
            msg = zmsg ? zmsg : "?";
            got = -1;
        }
    }
    if (got < 0) {
        s->pending = PCABI_E_PARSE;
        s->pending_msg = "read error: " + msg;
        s->eof = true;
        return 0;
    }
    if (got == 0) s->eof = true;
    s->end += (size_t)got;
    return got;
}

static void bam_fault(BamState *s, const std::string &what) {
    if (s->pending) return;
    s->pending = PCABI_E_PARSE;
    s->pending_msg = "read error: " + what;
    s->eof = true;
}

// Fills the empty stage with the next whole records. Leaves it empty at the end of the input or at a
// fault (s->pending). Returns 0, or a negative code for a device error.
static int bam_fill(pcabi_fastx *r) {
    using namespace pcabi_bam;
    BamState *s = r->bam;
    s->recs.clear();
    s->names.clear();
    s->name_off.assign(1, 0);
    s->aux.clear();
    s->stored.clear();
    s->aux_off.assign(1, 0);
    s->next = 0;
    Layout lay;
    while (s->recs.empty() && !s->pending) {
        // what the window holds: the header, then whole records from `at`
        if (!s->header_done) {
            const int64_t h = header_len(s->win.data(), (int64_t)s->end);
            if (h < 0) {
                bam_fault(s, s->end >= 4 && s->win[3] != 1 ? "BAM version byte " + std::to_string((int)s->win[3]) + " is not supported"
                                                           : std::string("invalid BAM header"));
                break;
            }
            if (h > 0) {
                s->header_done = true;
                s->at = (size_t)h;
                s->header_text.assign((const char *)s->win.data() + 8, (size_t)le32(s->win.data() + 4));
            }
        }
        if (s->header_done) {
            int64_t at = (int64_t)s->at;
            bool invalid = false, bad_aux = false;
            for (;;) {
                pcabi_bam_rec rec;
                int64_t size = 0;
                const int rc = record_at(s->win.data(), (int64_t)s->end, at, &rec, &size);
                if (rc <= 0) {
                    invalid = rc < 0;
                    break;
                }
                if (s->keep_aux && !(rec.flag & kSkipFlags)) {
                    const int64_t a0 = rec.seq_at + ((int64_t)rec.l_seq + 1) / 2 + rec.l_seq;
                    const uint8_t *ax = s->win.data() + at + a0;
                    if (!aux_walks(ax, size - a0)) {
                        bad_aux = true;
                        break;
                    }
                    s->aux.insert(s->aux.end(), ax, ax + (size - a0));
                    s->aux_off.push_back((int64_t)s->aux.size());
                    s->stored.push_back((rec.flag & kReverse) ? 0 : 1);
                }
                at += size;
                if (rec.flag & kSkipFlags) continue;
                lay.place(&rec);
                s->recs.push_back(rec);
                const char *nm = (const char *)s->win.data() + rec.rec + 4 + kFixed;
                s->names.insert(s->names.end(), nm, nm + rec.name_len);
                s->name_off.push_back((int64_t)s->names.size());
            }
            s->at = (size_t)at;
            if (invalid) bam_fault(s, "invalid BAM record at offset " + std::to_string(s->base + at));
            if (bad_aux) bam_fault(s, "invalid aux tags in the BAM record at offset " + std::to_string(s->base + at));
        }
        if (!s->recs.empty() || s->pending) break;
        // nothing whole in the window: more bytes behind the carried ones, or the end
        if (r->dev && s->header_done && s->end - s->at >= 4) {
            // the index knows the stream's length: a record that runs past it fails now, not after the
            // rest of the file has been carried into the window
            const int64_t block = le32(s->win.data() + s->at), rec_at = s->base + (int64_t)s->at;
            if (rec_at + 4 + block > s->total_est) {
                bam_fault(s, "truncated BAM record at offset " + std::to_string(rec_at));
                break;
            }
        }
        if (s->eof) {
            if (!s->header_done) bam_fault(s, "truncated BAM header");
            else if (s->at < s->end) bam_fault(s, "truncated BAM record at offset " + std::to_string(s->base + (int64_t)s->at));
            break;
        }
        const int64_t got = bam_refill(r);
        if (got < 0) return (int)got;
    }
    if (!s->recs.empty()) {
        if (s->dev) {
            if (int rc = pcabi_internal::bam_dev_unpack(s->dev, s->recs.data(), (int64_t)s->recs.size(), lay, &s->seq, &s->qual,
                                                        &s->codes))
                return rc;
        } else {
            s->h_seq.resize((size_t)lay.seq);
            s->h_qual.resize((size_t)lay.seq);
            s->h_codes.resize((size_t)lay.code);
            for (const pcabi_bam_rec &q : s->recs)
                unpack_range(s->win.data() + q.rec + q.seq_at, q.l_seq, q.flag, 0, q.l_seq, s->h_seq.data() + q.seq_out,
                             s->h_qual.data() + q.qual_out, s->h_codes.data() + q.code_out);
            s->seq = s->h_seq.data();
            s->qual = s->h_qual.data();
            s->codes = s->h_codes.data();
        }
    }
    return 0;
}

static int64_t bam_next(pcabi_fastx *r, int64_t max_reads, int64_t max_bases, pcabi_reads **out) {
    BamState *s = r->bam;
    pcabi_reads *b = new pcabi_reads();
    b->type = PCABI_FASTQ;
    int64_t bases = 0;
    while (b->n < max_reads && bases < max_bases) {
        if (s->next >= s->recs.size()) {
            if (int rc = bam_fill(r)) {
                delete b;
                return rc;
            }
            if (s->recs.empty()) break;   // the end of the input, or a fault
        }
        const size_t i = s->next;
        size_t j = i;
        while (j < s->recs.size() && b->n + (int64_t)(j - i) < max_reads && bases < max_bases) bases += s->recs[j++].l_seq;
        const pcabi_bam_rec &first = s->recs[i], &last = s->recs[j - 1];
        if (b->n == 0) {
            // room for the batch at once when it is large (growing gigabyte buffers by doubling copies
            // them twice over): the bases max_bases allows, but no more than the staged records and the
            // input behind the window can hold (a base takes a byte and a half of a record). A batch
            // that outgrows it grows as any vector does.
            const pcabi_bam_rec &end = s->recs.back();
            const int64_t staged = end.seq_out + end.l_seq - first.seq_out;
            const int64_t behind = std::max<int64_t>(0, s->total_est - s->base - (int64_t)s->end);
            const int64_t want = std::min(max_bases, staged + behind / 3 * 2);
            if (want >= (int64_t)bigmem::kBig) {   // smaller buffers come from malloc and grow cheaply
                b->seq.reserve((size_t)want);
                b->qual.reserve((size_t)want);
                b->codes.reserve((size_t)want + (size_t)want / 8);   // padding: at most 3 bytes a read
            }
        }
        const int64_t c0 = first.code_out, c1 = last.code_out + (((int64_t)last.l_seq + 3) & ~(int64_t)3);
        const int64_t code_base = (int64_t)b->codes.size();
        b->seq.insert(b->seq.end(), s->seq + first.seq_out, s->seq + last.seq_out + last.l_seq);
        b->qual.insert(b->qual.end(), s->qual + first.qual_out, s->qual + last.qual_out + last.l_seq);
        b->codes.insert(b->codes.end(), s->codes + c0, s->codes + c1);
        b->names.insert(b->names.end(), s->names.data() + s->name_off[i], s->names.data() + s->name_off[j]);
        for (size_t k = i; k < j; ++k) {
            const pcabi_bam_rec &q = s->recs[k];
            b->name_off.push_back(b->name_off.back() + (s->name_off[k + 1] - s->name_off[k]));
            b->seq_off.push_back(b->seq_off.back() + q.l_seq);
            b->qual_off.push_back(b->qual_off.back() + q.l_seq);
            b->spacer_off.push_back(0);
            b->rna.push_back(0);
            b->code_off.push_back(code_base + (q.code_out - c0));
            b->len.push_back(q.l_seq);
        }
        if (s->keep_aux) {
            if (b->aux_off.empty()) b->aux_off.push_back(0);
            b->aux.insert(b->aux.end(), s->aux.begin() + s->aux_off[i], s->aux.begin() + s->aux_off[j]);
            for (size_t k = i; k < j; ++k) {
                b->aux_off.push_back(b->aux_off.back() + (s->aux_off[k + 1] - s->aux_off[k]));
                b->as_stored.push_back(s->stored[k]);
            }
        }
        b->n += (int64_t)(j - i);
        s->next = j;
    }
    if (b->n == 0 && s->pending) {
        delete b;
        return fail(s->pending, s->pending_msg);
    }
    finish_batch(b);
    *out = b;
    return b->n;
}

int pcabi_fastx_load(const char *path, int raw, pcabi_reads **out) {
    if (!out) return fail(PCABI_E_ARG, "bad arguments");
    *out = nullptr;
    pcabi_fastx *r = nullptr;
    if (int rc = pcabi_fastx_open(path, raw, &r)) return rc;
    pcabi_reads *all = nullptr;
    int64_t got = pcabi_fastx_next(r, INT64_MAX, INT64_MAX, &all);
    if (got >= 0 && r->bam) {
        // a BAM reader delivers the records before a fault first: the fault is the next call's
        pcabi_reads *none = nullptr;
        const int64_t more = pcabi_fastx_next(r, 1, 1, &none);
        delete none;
        if (more < 0) {
            delete all;
            got = more;
        }
    }
    pcabi_fastx_close(r);
    if (got < 0) return (int)got;
    *out = all;
    return 0;
}

void pcabi_reads_free(pcabi_reads *b) { delete b; }

void pcabi_gather_host(const uint8_t *src, const int64_t *src_off, const int32_t *len, int64_t n, uint8_t *dst,
                       const int64_t *dst_off) {
    for (int64_t i = 0; i < n; ++i)
        if (len[i] > 0) std::memcpy(dst + dst_off[i], src + src_off[i], (size_t)len[i]);
}

void pcabi_encode_dna5_gather(const uint64_t *src, const int64_t *len, const int64_t *dst_off, int64_t n,
                              uint8_t *codes, int64_t codes_len) {
    static const struct Tab {
        uint8_t t[256];
        Tab() {
            for (int c = 0; c < 256; ++c) t[c] = 4;
            t['A'] = t['a'] = 0;
            t['C'] = t['c'] = 1;
            t['G'] = t['g'] = 2;
            t['T'] = t['t'] = t['U'] = t['u'] = 3;
        }
    } tab;
    // segments [lo, hi) and the N gap after each (up to the next segment / codes_len)
    auto run = [&](int64_t lo, int64_t hi) {
        if (lo == 0 && n > 0) std::memset(codes, 4, (size_t)dst_off[0]);
        for (int64_t i = lo; i < hi; ++i) {
            const uint8_t *s = reinterpret_cast<const uint8_t *>(src[i]);
            uint8_t *d = codes + dst_off[i];
            for (int64_t k = 0; k < len[i]; ++k) d[k] = tab.t[s[k]];
            const int64_t end = i + 1 < n ? dst_off[i + 1] : codes_len;
            const int64_t gap = end - dst_off[i] - len[i];
            if (gap > 0) std::memset(d + len[i], 4, (size_t)gap);
        }
    };
    if (n <= 0) {
        if (codes_len > 0) std::memset(codes, 4, (size_t)codes_len);
        return;
    }
    // split by bytes, not by segments: chunk k starts at the first segment at or past k/nt of the total
    const int nt = (int)std::min<int64_t>(16, std::max<int64_t>(1, codes_len / (4 << 20)));
    if (nt <= 1) {
        run(0, n);
        return;
    }
    std::vector<int64_t> cut(nt + 1, n);
    cut[0] = 0;
    for (int k = 1; k < nt; ++k)
        cut[k] = std::lower_bound(dst_off, dst_off + n, codes_len * k / nt) - dst_off;
    std::vector<std::thread> th;
    for (int k = 0; k < nt; ++k)
        if (cut[k] < cut[k + 1]) th.emplace_back(run, cut[k], cut[k + 1]);
    for (auto &t : th) t.join();
}

int pcabi_fastx_keep_aux(pcabi_fastx *r, int on) {
    if (!r) return fail(PCABI_E_ARG, "bad arguments");
    if (r->bam) r->bam->keep_aux = on != 0;
    return 0;
}

int pcabi_fastx_header_tags(pcabi_fastx *r, int on, int device) {
    if (!r) return fail(PCABI_E_ARG, "bad arguments");
    if (r->bam) return 0;   // a BAM reader's tags are its records' (pcabi_fastx_keep_aux)
    if (r->raw) return fail(PCABI_E_ARG, "a raw reader keeps the file's text and parses no tags");
    r->header_tags = on != 0;
    r->tags_device = device;
    if (r->header_tags && device >= 0 && !r->tags_dev) r->tags_dev = pcabi_internal::auxparse_dev_new();
    return 0;
}

int pcabi_fastx_bam_header(const pcabi_fastx *r, const char **text, int64_t *len) {
    if (!r || !text || !len) return fail(PCABI_E_ARG, "bad arguments");
    *text = r->bam ? r->bam->header_text.data() : "";
    *len = r->bam ? (int64_t)r->bam->header_text.size() : 0;
    return 0;
}

int pcabi_reads_aux(const pcabi_reads *b, const uint8_t **aux, const int64_t **aux_off, const uint8_t **as_stored) {
    if (!b || !aux || !aux_off || !as_stored) return fail(PCABI_E_ARG, "bad arguments");
    const bool have = !b->aux_off.empty();
    *aux = have ? b->aux.data() : nullptr;
    *aux_off = have ? b->aux_off.data() : nullptr;
    *as_stored = have ? b->as_stored.data() : nullptr;
    return 0;
}

int64_t pcabi_reads_count(const pcabi_reads *b) { return b ? b->n : 0; }
int pcabi_reads_type(const pcabi_reads *b) { return b ? b->type : -1; }

int pcabi_reads_views(const pcabi_reads *b, pcabi_reads_view *v) {
    if (!b || !v) return fail(PCABI_E_ARG, "bad arguments");
    v->n = b->n;
    v->type = b->type;
    v->names = b->names.data();
    v->name_off = b->name_off.data();
    v->seq = b->seq.data();
    v->seq_off = b->seq_off.data();
    v->qual = b->qual.data();
    v->qual_off = b->qual_off.data();
    v->rna = b->rna.data();
    v->spacer = b->spacer.data();
    v->spacer_off = b->spacer_off.data();
    v->codes = b->codes.data();
    v->codes_len = (int64_t)b->codes.size();
    v->code_off = b->code_off.data();
    v->len = b->len.data();
    return 0;
}

}  // extern "C"
