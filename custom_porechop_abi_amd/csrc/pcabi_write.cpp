// pcabi_write.cpp -- the writers of a batch of reads (host code, part of libpcabi.so; declared in
// include/pcabi.h; the batch and the io threads: csrc/pcabi_reads.h): FASTA / FASTQ text, unaligned BAM,
// and text with SAM tags in its headers.
// The text writer reproduces NanoporeRead.get_fasta / get_fastq (nanopore_read.py:106-156) for a
// batch: start / end trims with Python slice semantics, middle split parts (positions given as
// [begin, end) ranges of the trimmed sequence, parts shorter than min_split_read_size dropped,
// names numbered like add_number_to_read_name, :503-509), 70-column FASTA lines, T -> U for RNA
// reads, optional gzip. The other two write the same parts (read_parts) and share TagParts and the
// remap stage (pcabi_hostdev.h RemapHost / RemapDev) for the tags that count a read's bases.
#include <fcntl.h>
#include <sys/uio.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_auxtext.h"
#include "pcabi_bam.h"
#include "pcabi_deflate.h"
#include "pcabi_hostdev.h"
#include "pcabi_reads.h"

using pcabi_internal::fail;
using pcabi_internal::now_s;

// ---- files and clocks ------------------------------------------------------------------------
namespace {

// An output file, plain or zlib-compressed, that closes itself: open() with the append / truncate flags,
// write_all() in pieces of at most 256 MiB, close() tells whether everything went well (ok: so far).
struct OutFile {
    int fd = -1;
    gzFile gz = nullptr;
    bool ok = true;
    OutFile() = default;
    OutFile(const OutFile &) = delete;
    OutFile &operator=(const OutFile &) = delete;
    ~OutFile() { close(); }
    bool open(const char *path, int append, bool zlib = false) {
        if (zlib) gz = gzopen(path, append ? "ab" : "wb");
        else fd = ::open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0666);
        return gz || fd >= 0;
    }
    void write_all(const void *p, size_t n) {
        for (size_t k = 0; ok && k < n;) {
            const size_t piece = std::min<size_t>(n - k, 256u << 20);
            if (gz) {
                ok = gzwrite(gz, (const char *)p + k, (unsigned)piece) == (int)piece;
                k += piece;
                continue;
            }
            const ssize_t w = ::write(fd, (const char *)p + k, piece);
            if (w >= 0) k += (size_t)w;
            else if (errno != EINTR) ok = false;
        }
    }
    bool close() {
        if (gz && gzclose(gz) != Z_OK) ok = false;
        if (fd >= 0 && ::close(fd) != 0) ok = false;
        gz = nullptr, fd = -1;
        return ok;
    }
};

// The seconds the calling thread's last pcabi_reads_write* spent laying the records out (sizing, fill,
// block planning), compressing and writing the file (pcabi_reads_write_last_times): cleared when a call
// begins, and touched by nothing else.
struct WriteTimes {
    enum { kLayout, kCompress, kWrite };
    static double *last() { static thread_local double v[3] = {0, 0, 0}; return v; }
    double *const v = last();
    const double t_begin = now_s();
    WriteTimes() { v[0] = v[1] = v[2] = 0; }
    void layout_done() { v[kLayout] = now_s() - t_begin; }        // everything since the call began
    void add(int k, double t0) { v[k] += now_s() - t0; }          // the time since t0
    void write(OutFile &f, const void *p, size_t n) {              // p[0, n) to f, counted as writing
        const double t0 = now_s();
        f.write_all(p, n);
        add(kWrite, t0);
    }
    // a device path, begun at t0: `layout_s` of it were the host's layout, the device's share is what is left
    void device_done(double t0, double layout_s) {
        v[kLayout] += layout_s;
        v[kCompress] = now_s() - t0 - v[kWrite] - layout_s;
    }
};

}  // namespace

// ---- writer ----------------------------------------------------------------------------------
namespace {

// Output sink. Plain files are written with writev straight from the batch's buffers (one
// copy, into the page cache); only text the writer makes itself (numbered names, U for T, FASTA
// line breaks) is staged in an arena first. gzip / stdout go through a buffer.
struct Sink {
    FILE *fp = nullptr;
    gzFile gz = nullptr;
    int fd = -1;
    std::string buf;
    std::vector<iovec> iov;
    std::vector<std::unique_ptr<char[]>> arena;
    size_t arena_left = 0;
    char *arena_p = nullptr;
    bool ok = true;
    void flush() {
        if (fd >= 0) {
            size_t k = 0;
            while (ok && k < iov.size()) {
                const int cnt = (int)std::min<size_t>(iov.size() - k, 1024);
                const ssize_t w = ::writev(fd, iov.data() + k, cnt);
                if (w < 0) {
                    if (errno == EINTR) continue;
                    ok = false;
                    break;
                }
                size_t left = (size_t)w;   // advance past what was written (partial writes)
                while (left > 0 && k < iov.size()) {
                    if (left >= iov[k].iov_len) {
                        left -= iov[k].iov_len;
                        ++k;
                    } else {
                        iov[k].iov_base = (char *)iov[k].iov_base + left;
                        iov[k].iov_len -= left;
                        left = 0;
                    }
                }
            }
            iov.clear();
            arena.clear();
            arena_left = 0;
            return;
        }
        if (buf.empty()) return;
        if (gz) ok = ok && gzwrite(gz, buf.data(), (unsigned)buf.size()) == (int)buf.size();
        else ok = ok && std::fwrite(buf.data(), 1, buf.size(), fp) == buf.size();
        buf.clear();
    }
    // bytes that stay valid until the next flush (the batch, string literals)
    void ref(const char *p, size_t n) {
        if (n == 0) return;
        if (fd < 0) {
            put(p, n);
            return;
        }
        iov.push_back(iovec{const_cast<char *>(p), n});
        if (iov.size() >= 8192) flush();
    }
    // bytes the caller may reuse: copied
    void put(const char *p, size_t n) {
        if (n == 0) return;
        if (fd >= 0) {
            if (n > arena_left) {
                const size_t sz = std::max<size_t>(n, 1 << 20);
                arena.emplace_back(new char[sz]);
                arena_p = arena.back().get();
                arena_left = sz;
            }
            std::memcpy(arena_p, p, n);
            iov.push_back(iovec{arena_p, n});
            arena_p += n;
            arena_left -= n;
            if (iov.size() >= 8192) flush();
            return;
        }
        buf.append(p, n);
        if (buf.size() > (8u << 20)) flush();
    }
    void put(const std::string &s) { put(s.data(), s.size()); }
    void put(char c) { put(&c, 1); }
};

// Python seq[start:end] with start >= 0 and end possibly negative (counts from the end).
inline void py_slice(int64_t len, int64_t start, int64_t end, int64_t *a, int64_t *b) {
    if (end < 0) end = std::max<int64_t>(0, len + end);
    if (end > len) end = len;
    if (start > len) start = len;
    *a = start;
    *b = std::max(start, end);
}

std::string numbered(const char *name, size_t nn, int k) {
    std::string s(name, nn);
    const std::string tag = "_" + std::to_string(k);
    size_t p = s.find('\t');
    if (p != std::string::npos) return s.substr(0, p) + tag + s.substr(p);
    p = s.find(' ');
    if (p != std::string::npos) return s.substr(0, p) + tag + s.substr(p);
    return s + tag;
}

// The parallel writer's two passes (pcabi_reads_write, plain files): CountSink sizes a range of
// records, MemSink copies them to their place in one contiguous output buffer.
struct CountSink {
    size_t n = 0;
    void ref(const char *, size_t k) { n += k; }
    void put(const char *, size_t k) { n += k; }
    void put(const std::string &x) { n += x.size(); }
    void put(char) { ++n; }
};
struct MemSink {
    char *p;
    void ref(const char *s, size_t k) {
        std::memcpy(p, s, k);
        p += k;
    }
    void put(const char *s, size_t k) { ref(s, k); }
    void put(const std::string &x) { ref(x.data(), x.size()); }
    void put(char c) { *p++ = c; }
};

template <class S>
void put_seq(S &o, const char *s, size_t n, bool rna, bool fasta) {
    std::string t;
    if (rna) {   // T -> U (a copy); otherwise the batch's bytes go out as they are
        t.assign(s, n);
        for (char &c : t)
            if (c == 'T') c = 'U';
        s = t.data();
    }
    if (!fasta) {
        if (rna) o.put(s, n);
        else o.ref(s, n);
        return;
    }
    for (size_t p = 0; p < n; p += 70) {   // add_line_breaks_to_sequence(seq, 70)
        if (rna) o.put(s + p, std::min<size_t>(70, n - p));
        else o.ref(s + p, std::min<size_t>(70, n - p));
        o.ref("\n", 1);
    }
}

// name: the batch's own header bytes (stable) or a numbered copy (own = true)
template <class S>
void put_record(S &o, bool fasta, const char *name, size_t nn, bool own, const char *s, size_t ns,
                const char *q, size_t nq, bool rna) {
    o.ref(fasta ? ">" : "@", 1);
    if (own) o.put(name, nn);
    else o.ref(name, nn);
    o.ref("\n", 1);
    if (fasta) {
        put_seq(o, s, ns, rna, true);
    } else {
        put_seq(o, s, ns, rna, false);
        o.ref("\n+\n", 3);
        o.ref(q, nq);
        o.ref("\n", 1);
    }
}

// What a writer is asked for (pcabi_reads_write's arguments), and the part enumeration the text writers
// and the BAM writer share: part(name, name_len, own, s0, ns, q0, nq) is called for every record read i
// gives, in output order -- name: the batch's own header bytes (stable) or a numbered copy (own = true);
// [s0, s0 + ns) of the read's sequence, [q0, q0 + nq) of its qualities. Returns whether the read
// produced any output (the reference counts a read into its bin only then, porechop_abi.py:598-604).
struct WriteArgs {
    const pcabi_reads *b;
    const int32_t *start_trim, *end_trim;
    const int64_t *cut_off, *cuts;
    int min_split_read_size, discard_middle, untrimmed;
    const uint8_t *select;
};

template <class F>
bool read_parts(const WriteArgs &w, int64_t i, std::vector<std::pair<int64_t, int64_t>> &rg, F &&part) {
    const pcabi_reads *b = w.b;
    const int64_t *cut_off = w.cut_off, *cuts = w.cuts;
    if (w.select && !w.select[i]) return false;
    const char *name = b->names.data() + b->name_off[i];
    const size_t nn = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const int64_t ns = b->seq_off[i + 1] - b->seq_off[i];
    const int64_t nq = b->qual_off[i + 1] - b->qual_off[i];
    const int64_t st = w.start_trim ? w.start_trim[i] : 0, et = w.end_trim ? w.end_trim[i] : 0;
    // get_seq_with_start_end_adapters_trimmed / get_quals_... (nanopore_read.py:66-82)
    int64_t sa = 0, sb = ns, qa = 0, qb = nq;
    if (st || et) {
        py_slice(ns, st, ns - et, &sa, &sb);
        py_slice(nq, st, nq - et, &qa, &qb);
    }
    bool split = false;
    if (cut_off)
        for (int64_t k = cut_off[i]; k < cut_off[i + 1] && !split; ++k) split = cuts[2 * k + 1] > cuts[2 * k];
    if (!split) {
        if (w.untrimmed) { sa = 0; sb = ns; qa = 0; qb = nq; }
        if (sb == sa) return false;   // no empty sequences
        part(name, nn, false, sa, sb - sa, qa, qb - qa);
        return true;
    }
    if (w.discard_middle) return false;
    // split parts (get_split_read_parts, nanopore_read.py:84-104): positions of the trimmed
    // sequence inside any cut range are dropped
    rg.clear();
    for (int64_t k = cut_off[i]; k < cut_off[i + 1]; ++k)
        if (cuts[2 * k + 1] > cuts[2 * k]) rg.emplace_back(cuts[2 * k], cuts[2 * k + 1]);
    std::sort(rg.begin(), rg.end());
    const int64_t tl = sb - sa;
    int n_part = 0;
    size_t ri = 0;
    int64_t run = 0;   // start of the current kept run
    auto emit = [&](int64_t a, int64_t e) {
        if (e - a <= 0 || e - a < w.min_split_read_size) return;
        ++n_part;
        const std::string nm = numbered(name, nn, n_part);
        part(nm.data(), nm.size(), true, sa + a, e - a, qa + a, e - a);
    };
    int64_t pos = 0;
    while (pos < tl) {
        while (ri < rg.size() && rg[ri].second <= pos) ++ri;
        if (ri < rg.size() && rg[ri].first <= pos) {   // pos is cut
            emit(run, pos);
            int64_t e = rg[ri].second;
            for (size_t rj = ri; rj < rg.size() && rg[rj].first <= e; ++rj) e = std::max(e, rg[rj].second);
            pos = std::min(e, tl);
            run = pos;
        } else {
            const int64_t nxt = ri < rg.size() ? std::min(rg[ri].first, tl) : tl;
            pos = nxt;
        }
    }
    emit(run, tl);
    return n_part > 0;
}

}  // namespace

static int reads_write_impl(const pcabi_reads *b, const char *path, int append, int gz, int fasta,
                            const int32_t *start_trim, const int32_t *end_trim, const int64_t *cut_off,
                            const int64_t *cuts, int min_split_read_size, int discard_middle,
                            int untrimmed, const uint8_t *select, int gzip_device, bool bgzf) {
    // bgzf (with gz = 2): one indexed BGZF member per block of at most 65280 bytes, no end marker
    if (!b || !path) return fail(PCABI_E_ARG, "bad arguments");
    if (gz == 2 && std::strcmp(path, "-") == 0) return fail(PCABI_E_ARG, "gz = 2 writes files, not stdout");
    Sink o;
    OutFile file;   // o writes to it
    if (gz == 0 && std::strcmp(path, "-") == 0) {
        o.fp = stdout;
    } else {   // any non-zero value but 2 keeps meaning zlib
        if (!file.open(path, append, gz != 0 && gz != 2)) return fail(PCABI_E_ARG, std::string("could not write ") + path);
        o.gz = file.gz, o.fd = file.fd;
    }
    const WriteArgs wa{b, start_trim, end_trim, cut_off, cuts, min_split_read_size, discard_middle, untrimmed, select};
    auto format = [&](int64_t i, auto &o, std::vector<std::pair<int64_t, int64_t>> &rg) -> bool {
        const char *seq = b->seq.data() + b->seq_off[i], *qual = b->qual.data() + b->qual_off[i];
        const bool rna = b->rna[i] != 0;
        return read_parts(wa, i, rg, [&](const char *name, size_t nn, bool own, int64_t s0, int64_t ns, int64_t q0, int64_t nq) {
            put_record(o, fasta != 0, name, nn, own, seq + s0, (size_t)ns, qual + q0, (size_t)nq, rna);
        });
    };
    // One stream: the page-cache copy is the cost, and writers of one file serialise on its
    // inode (measured: threads writing disjoint ranges with pwritev were no faster). r05: a plain
    // file's records are first laid out in one contiguous buffer by the io threads (a sizing pass,
    // then each thread copies its range of records to its offset), then written in large write()
    // calls -- a writev of ~7 small pieces per record spent more on the pieces than on the bytes
    // (e2e writer 8.1 GB/s against 11.9 for one contiguous buffer, bench write_probe).
    int64_t emitted = 0;
    WriteTimes wt;
    const int nt = (int)std::min<int64_t>((int64_t)io_threads(), std::max<int64_t>(1, b->n / 512));
    // gz = 2: the same buffer, cut into blocks at line ends by the thread that filled each range
    // (pcabi_deflate.h plan_blocks), compressed on the device and written as gzip members.
    std::vector<char, NoInit<char>> out;
    std::vector<std::vector<int64_t>> ends((size_t)std::max(nt, 1));
    if (o.fd >= 0 && b->n > 0) {
        std::vector<int64_t> lo((size_t)nt + 1), bytes((size_t)nt + 1, 0), emit((size_t)nt, 0);
        for (int t = 0; t <= nt; ++t) lo[(size_t)t] = b->n * t / nt;
        fan_out(nt, [&](int t) {
            std::vector<std::pair<int64_t, int64_t>> rg;
            CountSink c;
            for (int64_t i = lo[(size_t)t]; i < lo[(size_t)t + 1]; ++i) format(i, c, rg);
            bytes[(size_t)t + 1] = (int64_t)c.n;
        });
        for (int t = 0; t < nt; ++t) bytes[(size_t)t + 1] += bytes[(size_t)t];
        out.resize((size_t)bytes[(size_t)nt]);
        fan_out(nt, [&](int t) {
            std::vector<std::pair<int64_t, int64_t>> rg;
            MemSink m{out.data() + bytes[(size_t)t]};
            int64_t e = 0;
            for (int64_t i = lo[(size_t)t]; i < lo[(size_t)t + 1]; ++i) e += format(i, m, rg) ? 1 : 0;
            emit[(size_t)t] = e;
            if (gz == 2)
                pcabi_deflate::plan_blocks(out.data(), bytes[(size_t)t], bytes[(size_t)t + 1], PCABI_GZIP_LONG_LINE,
                                           bgzf ? (int64_t)PCABI_BGZF_BLOCK_CAP : (int64_t)PCABI_GZIP_BLOCK_CAP,
                                           [&](int64_t end) { ends[(size_t)t].push_back(end); });
        });
        for (int t = 0; t < nt; ++t) emitted += emit[(size_t)t];
        wt.layout_done();
        if (gz != 2) wt.write(file, out.data(), out.size());
    } else {
        std::vector<std::pair<int64_t, int64_t>> rg;
        for (int64_t i = 0; i < b->n; ++i) emitted += format(i, o, rg) ? 1 : 0;
    }
    if (gz == 2) {
        std::vector<int64_t> block_off{0};
        for (const auto &v : ends) block_off.insert(block_off.end(), v.begin(), v.end());
        const int64_t nblk = (int64_t)block_off.size() - 1;
        std::vector<uint8_t, NoInit<uint8_t>> z;
        z.resize((size_t)(bgzf ? pcabi_bgzf_bound((int64_t)out.size(), std::max<int64_t>(nblk, 1), 0)
                               : pcabi_gzip_bound((int64_t)out.size(), std::max<int64_t>(nblk, 1))));
        const double t0 = now_s();
        const int64_t zn = bgzf ? pcabi_bgzf_host(gzip_device, (const uint8_t *)out.data(), (int64_t)out.size(),
                                                  block_off.data(), nblk, 0, z.data(), (int64_t)z.size())
                                : pcabi_gzip_host(gzip_device, (const uint8_t *)out.data(), (int64_t)out.size(),
                                                  block_off.data(), nblk, z.data(), (int64_t)z.size());
        wt.add(wt.kCompress, t0);
        if (zn < 0 || zn > (int64_t)z.size()) return zn < 0 ? (int)zn : fail(PCABI_E_ARG, "gzip capacity bound exceeded");
        wt.write(file, z.data(), (size_t)zn);
    }
    o.flush();
    const bool ok = o.ok && file.ok;   // what closing the file says is not looked at here
    file.close();
    if (o.fp) std::fflush(o.fp);
    if (!ok) return fail(PCABI_E_ARG, std::string("write failed: ") + path);
    return (int)std::min<int64_t>(emitted, INT32_MAX);
}

extern "C" int pcabi_reads_write(const pcabi_reads *b, const char *path, int append, int gz, int fasta,
                                 const int32_t *start_trim, const int32_t *end_trim, const int64_t *cut_off,
                                 const int64_t *cuts, int min_split_read_size, int discard_middle,
                                 int untrimmed, const uint8_t *select) {
    return reads_write_impl(b, path, append, gz, fasta, start_trim, end_trim, cut_off, cuts, min_split_read_size,
                            discard_middle, untrimmed, select, -1, false);
}

extern "C" int pcabi_reads_write_dev(const pcabi_reads *b, const char *path, int append, int gz, int fasta,
                                     const int32_t *start_trim, const int32_t *end_trim, const int64_t *cut_off,
                                     const int64_t *cuts, int min_split_read_size, int discard_middle,
                                     int untrimmed, const uint8_t *select, int gzip_device) {
    return reads_write_impl(b, path, append, gz == 3 ? 2 : gz, fasta, start_trim, end_trim, cut_off, cuts,
                            min_split_read_size, discard_middle, untrimmed, select, gzip_device, gz == 3);
}

extern "C" void pcabi_reads_write_last_times(double *layout, double *compress, double *write) {
    const double *t = WriteTimes::last();
    if (layout) *layout = t[0];
    if (compress) *compress = t[1];
    if (write) *write = t[2];
}

// ---- BAM writer ------------------------------------------------------------------------------
namespace {

// One BGZF member of data[0, n) (n <= 65280) appended to z: zlib raw deflate, stored when that fails to fit.
bool bgzf_member(const uint8_t *data, size_t n, std::vector<uint8_t> &z) {
    uint8_t body[PCABI_BGZF_MEMBER_MAX];
    size_t zn = 0;
    for (int level : {Z_DEFAULT_COMPRESSION, 0}) {
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        zs.next_in = const_cast<Bytef *>(data);
        zs.avail_in = (uInt)n;
        zs.next_out = body;
        zs.avail_out = (uInt)(PCABI_BGZF_MEMBER_MAX - 26);
        const int rc = deflate(&zs, Z_FINISH);
        zn = zs.total_out;
        deflateEnd(&zs);
        if (rc == Z_STREAM_END) break;
        if (level == 0) return false;
    }
    const uint32_t bsize = (uint32_t)(zn + 26 - 1), crc = (uint32_t)crc32(crc32(0, nullptr, 0), data, (uInt)n), isize = (uint32_t)n;
    const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
    z.insert(z.end(), hdr, hdr + 18);
    z.insert(z.end(), body, body + zn);
    for (uint32_t v : {crc, isize})
        for (int k = 0; k < 4; ++k) z.push_back((uint8_t)(v >> (8 * k)));
    return true;
}

// an integer tag's value (types c C s S i I), or INT64_MIN for any other type
int64_t aux_int(const uint8_t *tg) {
    using namespace pcabi_bam;
    switch (tg[2]) {
        case 'c': return (int8_t)tg[3];
        case 'C': return tg[3];
        case 's': return (int16_t)le16(tg + 3);
        case 'S': return le16(tg + 3);
        case 'i': return le32(tg + 3);
        case 'I': return (uint32_t)le32(tg + 3);
        default: return INT64_MIN;
    }
}

// fn(tag, next) for every tag of the chain ax[0, an), `next` the offset behind it; stops where the chain breaks
template <class F>
void each_tag(const uint8_t *ax, int64_t an, F &&fn) {
    for (int64_t at = 0, nx; at < an && (nx = pcabi_bam::aux_next(ax, an, at)) >= 0; at = nx) fn(ax + at, nx);
}

// The modification tags of one read's aux chain (include/pcabi.h pcabi_mods_read): -1 when it carries
// none of MM ML MN Mm Ml; else its entry appended to *reads, the MM text and the ML values named where
// they lie in the batch's aux bytes (the chain is aux[a0, a1)). What only the chain can tell -- not exactly
// one MM tag, a tag of the wrong type, a tag twice -- marks the read PCABI_MODS_BAD.
int64_t mods_read_of(const uint8_t *aux, int64_t a0, int64_t a1, int64_t seq_off, int64_t l_seq, std::vector<pcabi_mods_read> *reads,
                     int64_t part0) {
    const uint8_t *ax = aux + a0;
    const int64_t an = a1 - a0;
    pcabi_mods_read r;
    std::memset(&r, 0, sizeof r);
    r.seq_off = seq_off, r.part0 = part0, r.l_seq = (int32_t)l_seq;
    r.mm_len = r.ml_len = r.mn = -1;
    int n_mm = 0, n_ml = 0, n_mn = 0;
    bool any = false;
    each_tag(ax, an, [&](const uint8_t *tg, int64_t nx) {
        const int64_t at = tg - ax;
        if (tg[0] == 'M' && (tg[1] == 'M' || tg[1] == 'm')) {
            any = true;
            if (++n_mm > 1 || tg[2] != 'Z') r.flags |= PCABI_MODS_BAD;
            else {
                r.mm_off = a0 + at + 3, r.mm_len = (int32_t)(nx - at - 4);
                if (tg[1] == 'm') r.flags |= PCABI_MODS_OLD_MM;
            }
        } else if (tg[0] == 'M' && (tg[1] == 'L' || tg[1] == 'l')) {
            any = true;
            if (++n_ml > 1 || tg[2] != 'B' || tg[3] != 'C') r.flags |= PCABI_MODS_BAD;
            else {
                r.ml_off = a0 + at + 8, r.ml_len = (int32_t)(nx - at - 8);
                if (tg[1] == 'l') r.flags |= PCABI_MODS_OLD_ML;
            }
        } else if (tg[0] == 'M' && tg[1] == 'N') {
            any = true;
            const int64_t v = aux_int(tg);
            if (++n_mn > 1 || v < 0 || v > INT32_MAX) r.flags |= PCABI_MODS_BAD;
            else r.mn = (int32_t)v;
        }
    });
    if (!any) return -1;
    if (n_mm != 1) r.flags |= PCABI_MODS_BAD;
    reads->push_back(r);
    return (int64_t)reads->size() - 1;
}

// The move table of one read's aux chain (include/pcabi.h pcabi_moves_read): -1 when it carries no mv
// tag; else its entry appended to *reads. What only the chain can tell -- mv twice or not of type B:c /
// B:C, ts twice, not an integer, negative or above INT32_MAX -- marks the read PCABI_MOVES_BAD.
int64_t moves_read_of(const uint8_t *aux, int64_t a0, int64_t a1, int64_t l_seq, std::vector<pcabi_moves_read> *reads, int64_t part0) {
    using namespace pcabi_bam;
    const uint8_t *ax = aux + a0;
    const int64_t an = a1 - a0;
    pcabi_moves_read r;
    std::memset(&r, 0, sizeof r);
    r.part0 = part0, r.l_seq = (int32_t)l_seq, r.ts = -1;
    int n_mv = 0, n_ts = 0;
    each_tag(ax, an, [&](const uint8_t *tg, int64_t) {
        if (tg[0] == 'm' && tg[1] == 'v') {
            const uint32_t count = tg[2] == 'B' ? (uint32_t)le32(tg + 4) : 0;
            if (++n_mv > 1 || tg[2] != 'B' || (tg[3] != 'c' && tg[3] != 'C') || count > (uint32_t)INT32_MAX - 64) r.flags |= PCABI_MOVES_BAD;
            else r.mv_off = a0 + (tg - ax) + 8, r.n_vals = (int32_t)count;
        } else if (tg[0] == 't' && tg[1] == 's') {
            const int64_t v = aux_int(tg);
            if (++n_ts > 1 || v < 0 || v > INT32_MAX) r.flags |= PCABI_MOVES_BAD;
            else r.ts = (int32_t)v;
        }
    });
    if (n_mv == 0) return -1;
    if (r.flags & PCABI_MOVES_BAD) r.mv_off = 0, r.n_vals = 0;
    reads->push_back(r);
    return (int64_t)reads->size() - 1;
}

// What the BAM writer and the text writer with tags in its headers (pcabi_reads_write_tags) share: the
// parts of a batch, the tables of the tags to remap, and the side blob (per part its name, then its aux
// bytes) with a gap behind each part's kept tags for what is remapped.
struct TagParts {
    const pcabi_reads *b;
    const WriteArgs &wa;
    const bool have_aux, remap, keep_moves, no_qual;
    const int nt;
    // the changed reads that carry modification tags and their parts (include/pcabi.h pcabi_mods_*; the tag
    // blob is the batch's aux bytes), per thread's range of reads, then joined
    std::vector<pcabi_mods_read> mreads;
    std::vector<pcabi_mods_part> mparts;
    std::vector<int64_t> mpart0;   // a thread's first entry of mparts
    std::vector<uint8_t> has_mods;
    // the same for the move tables (pcabi_moves_*): vread[i] = the read's entry of vreads, -1 without one
    std::vector<pcabi_moves_read> vreads;
    std::vector<pcabi_moves_part> vparts;
    std::vector<int64_t> vpart0;
    std::vector<int32_t> vread;
    std::vector<uint8_t> usable, vusable;
    pcabi_internal::ModsTables mt;
    pcabi_internal::MovesTables vt;
    // what layout() makes
    std::vector<pcabi_bam_part> parts;
    std::vector<uint8_t> side;
    std::vector<int32_t> kept;      // per part: the aux bytes that lie before its gaps
    std::vector<int64_t> tpart0;    // a thread's first entry of parts
    int64_t emitted = 0;

    TagParts(const pcabi_reads *b_, const WriteArgs &wa_, int keep_aux, int tag_flags)
        : b(b_), wa(wa_), have_aux(keep_aux && !b_->aux_off.empty()), remap(have_aux && keep_aux == 2),
          keep_moves(have_aux && (tag_flags & PCABI_BAM_KEEP_MOVES)), no_qual(b_->type == PCABI_FASTA),
          nt((int)std::min<int64_t>((int64_t)io_threads(), std::max<int64_t>(1, b_->n / 512))) {}
    // the tables of a kind, null when no read has such tags to remap
    const pcabi_internal::ModsTables *mods() const { return mreads.empty() ? nullptr : &mt; }
    const pcabi_internal::MovesTables *moves() const { return vreads.empty() ? nullptr : &vt; }
    // A part keeps its read's aux bytes verbatim when it is the whole read with the bases as stored.
    bool verbatim(int64_t i, bool own, int64_t s0, int64_t ns) const {
        return !own && s0 == 0 && ns == b->seq_off[i + 1] - b->seq_off[i] && b->as_stored[i];
    }

    // first pass: the tables of the tags to remap
    void list() {
        mpart0.assign((size_t)nt + 1, 0);
        vpart0.assign((size_t)nt + 1, 0);
        has_mods.assign(remap ? (size_t)b->n : 0, 0);
        vread.assign(keep_moves ? (size_t)b->n : 0, -1);
        if (remap || keep_moves) {
            std::vector<std::vector<pcabi_mods_read>> t_reads((size_t)nt);
            std::vector<std::vector<pcabi_mods_part>> t_parts((size_t)nt);
            std::vector<std::vector<pcabi_moves_read>> t_vreads((size_t)nt);
            std::vector<std::vector<pcabi_moves_part>> t_vparts((size_t)nt);
            fan_out(nt, [&](int t) {
                std::vector<std::pair<int64_t, int64_t>> rg;
                for (int64_t i = b->n * t / nt; i < b->n * (t + 1) / nt; ++i) {
                    int64_t mread = -2, mv = -2;   // the read's entry; -1: it carries none of the tags; -2: not looked yet
                    read_parts(wa, i, rg, [&](const char *, size_t, bool own, int64_t s0, int64_t ns, int64_t, int64_t) {
                        if (verbatim(i, own, s0, ns)) return;
                        if (remap && mread == -2)
                            mread = mods_read_of(b->aux.data(), b->aux_off[i], b->aux_off[i + 1], b->seq_off[i],
                                                 b->seq_off[i + 1] - b->seq_off[i], &t_reads[(size_t)t], (int64_t)t_parts[(size_t)t].size());
                        if (keep_moves && mv == -2)
                            mv = moves_read_of(b->aux.data(), b->aux_off[i], b->aux_off[i + 1], b->seq_off[i + 1] - b->seq_off[i],
                                               &t_vreads[(size_t)t], (int64_t)t_vparts[(size_t)t].size());
                        if (keep_moves && mv >= 0) {
                            vread[(size_t)i] = (int32_t)mv;
                            ++t_vreads[(size_t)t][(size_t)mv].n_parts;
                            t_vparts[(size_t)t].push_back(pcabi_moves_part{0, (int32_t)mv, (int32_t)s0, (int32_t)ns, 0});
                        }
                        if (!remap || mread < 0) return;
                        has_mods[(size_t)i] = 1;
                        ++t_reads[(size_t)t][(size_t)mread].n_parts;
                        t_parts[(size_t)t].push_back(pcabi_mods_part{0, (int32_t)mread, (int32_t)s0, (int32_t)ns, 0});
                    });
                }
            });
            for (int t = 0; t < nt; ++t) {
                const int64_t read_base = join(t_vreads[(size_t)t], t_vparts[(size_t)t], &vreads, &vparts, &vpart0[(size_t)t]);
                if (keep_moves)
                    for (int64_t i = b->n * t / nt; i < b->n * (t + 1) / nt; ++i)
                        if (vread[(size_t)i] >= 0) vread[(size_t)i] += (int32_t)read_base;
                join(t_reads[(size_t)t], t_parts[(size_t)t], &mreads, &mparts, &mpart0[(size_t)t]);
            }
            vpart0[(size_t)nt] = (int64_t)vparts.size();
            mpart0[(size_t)nt] = (int64_t)mparts.size();
        }
        usable.assign(mreads.size(), 0);
        vusable.assign(vreads.size(), 0);
        const int64_t aux_n = (int64_t)b->aux.size();
        mt = {b->aux.data(), aux_n, mreads.data(), (int64_t)mreads.size(), mparts.data(), (int64_t)mparts.size(), usable.data()};
        vt = {b->aux.data(), aux_n, vreads.data(), (int64_t)vreads.size(), vparts.data(), (int64_t)vparts.size(), vusable.data()};
    }
    // a thread's tables appended to the joined ones: *part0 = where its parts begin there, its reads' part0
    // and its parts' read moved along; returns where its reads begin
    template <class R, class P>
    static int64_t join(const std::vector<R> &t_reads, const std::vector<P> &t_parts, std::vector<R> *reads, std::vector<P> *parts,
                        int64_t *part0) {
        const int64_t read_base = (int64_t)reads->size(), part_base = (int64_t)parts->size();
        *part0 = part_base;
        for (R r : t_reads) {
            r.part0 += part_base;
            reads->push_back(r);
        }
        for (P p : t_parts) {
            p.read += (int32_t)read_base;
            parts->push_back(p);
        }
        return read_base;
    }

    // The parts and their side blob (name, then aux bytes), per thread's range of reads, then joined. With
    // sized modification tags (mparts[].len) a gap of the tags' length follows a part's kept tags, and
    // mparts[].out names it; a gap for a sized move table (vparts[].len, mv then ts) follows that, and a
    // read whose ts is rewritten there loses it from the kept tags.
    void layout() {
        using namespace pcabi_bam;
        std::vector<std::vector<pcabi_bam_part>> t_parts((size_t)nt);
        std::vector<std::vector<uint8_t>> t_side((size_t)nt);
        std::vector<std::vector<int32_t>> t_kept((size_t)nt);
        std::vector<int64_t> t_emit((size_t)nt, 0);
        fan_out(nt, [&](int t) {
            std::vector<std::pair<int64_t, int64_t>> rg;
            std::vector<pcabi_bam_part> &parts = t_parts[(size_t)t];
            std::vector<uint8_t> &side = t_side[(size_t)t];
            int64_t mp = mpart0[(size_t)t], vp = vpart0[(size_t)t];
            for (int64_t i = b->n * t / nt; i < b->n * (t + 1) / nt; ++i) {
                t_emit[(size_t)t] += read_parts(wa, i, rg, [&](const char *name, size_t nn, bool own, int64_t s0, int64_t ns, int64_t q0, int64_t nq) {
                    pcabi_bam_part p;
                    std::memset(&p, 0, sizeof p);
                    p.seq_src = b->seq_off[i] + s0;
                    p.qual_src = (no_qual || nq < ns) ? -1 : b->qual_off[i] + q0;
                    p.side_off = (int64_t)side.size();
                    p.l_seq = (int32_t)ns;
                    // the name: the header up to its first space or tab, at most 254 bytes, "*" when empty
                    size_t k = 0;
                    while (k < nn && k < (size_t)kMaxName && name[k] != ' ' && name[k] != '\t') ++k;
                    if (k == 0) side.push_back('*'), k = 1;
                    else side.insert(side.end(), name, name + k);
                    p.name_len = (int32_t)k;
                    int32_t kept_len = 0;
                    if (have_aux) {
                        const uint8_t *ax = b->aux.data() + b->aux_off[i];
                        const int64_t an = b->aux_off[i + 1] - b->aux_off[i];
                        if (verbatim(i, own, s0, ns)) {
                            side.insert(side.end(), ax, ax + an);   // the whole read, as stored
                            kept_len = (int32_t)an;
                        } else {   // a changed read: without the tags that count its bases
                            const int32_t vr = keep_moves ? vread[(size_t)i] : -1;
                            const bool new_ts = vr >= 0 && vusable[(size_t)vr] && vreads[(size_t)vr].ts >= 0;
                            each_tag(ax, an, [&](const uint8_t *tg, int64_t nx) {
                                if (!aux_positional(tg) && !(new_ts && tg[0] == 't' && tg[1] == 's')) side.insert(side.end(), tg, ax + nx);
                            });
                            kept_len = (int32_t)((int64_t)side.size() - p.side_off - p.name_len);
                            if (remap && has_mods[(size_t)i]) {   // its remapped tags go behind them
                                mparts[(size_t)mp].out = (int64_t)side.size();
                                side.resize(side.size() + (size_t)mparts[(size_t)mp].len);
                                ++mp;
                            }
                            if (vr >= 0) {   // and its move table behind those
                                vparts[(size_t)vp].out = (int64_t)side.size();
                                side.resize(side.size() + (size_t)vparts[(size_t)vp].len);
                                ++vp;
                            }
                        }
                        p.aux_len = (int32_t)((int64_t)side.size() - p.side_off - p.name_len);
                    }
                    t_kept[(size_t)t].push_back(kept_len);
                    parts.push_back(p);
                }) ? 1 : 0;
            }
        });
        tpart0.assign((size_t)nt + 1, 0);
        for (int t = 0; t < nt; ++t) {
            const int64_t base = (int64_t)side.size();
            tpart0[(size_t)t] = (int64_t)parts.size();
            for (pcabi_bam_part p : t_parts[(size_t)t]) {
                p.side_off += base;
                parts.push_back(p);
            }
            kept.insert(kept.end(), t_kept[(size_t)t].begin(), t_kept[(size_t)t].end());
            for (int64_t m = mpart0[(size_t)t]; m < mpart0[(size_t)t + 1]; ++m) mparts[(size_t)m].out += base;
            for (int64_t m = vpart0[(size_t)t]; m < vpart0[(size_t)t + 1]; ++m) vparts[(size_t)m].out += base;
            side.insert(side.end(), t_side[(size_t)t].begin(), t_side[(size_t)t].end());
            t_side[(size_t)t] = std::vector<uint8_t>();
            emitted += t_emit[(size_t)t];
        }
        tpart0[(size_t)nt] = (int64_t)parts.size();
    }
};

}  // namespace

extern "C" int pcabi_reads_write_bam(const pcabi_reads *b, const char *path, int append, const int32_t *start_trim,
                                     const int32_t *end_trim, const int64_t *cut_off, const int64_t *cuts,
                                     int min_split_read_size, int discard_middle, int untrimmed, const uint8_t *select,
                                     const char *header_text, int64_t header_len, int keep_aux, int device) {
    return pcabi_reads_write_bam_tags(b, path, append, start_trim, end_trim, cut_off, cuts, min_split_read_size, discard_middle, untrimmed,
                                      select, header_text, header_len, keep_aux, 0, device);
}

extern "C" int pcabi_reads_write_bam_tags(const pcabi_reads *b, const char *path, int append, const int32_t *start_trim,
                                          const int32_t *end_trim, const int64_t *cut_off, const int64_t *cuts,
                                          int min_split_read_size, int discard_middle, int untrimmed, const uint8_t *select,
                                          const char *header_text, int64_t header_len, int keep_aux, int tag_flags, int device) {
    using namespace pcabi_bam;
    if (tag_flags & ~PCABI_BAM_KEEP_MOVES) return fail(PCABI_E_ARG, "unknown tag_flags");
    if (!b || !path || header_len < 0 || header_len > INT32_MAX - 16 || (header_len > 0 && !header_text))
        return fail(PCABI_E_ARG, "bad arguments");
    if (std::strcmp(path, "-") == 0) return fail(PCABI_E_ARG, "BAM output goes to files, not stdout");
    WriteTimes wt;
    const WriteArgs wa{b, start_trim, end_trim, cut_off, cuts, min_split_read_size, discard_middle, untrimmed, select};
    // the tables of the tags to remap (TagParts::list), then the parts and their side blob (TagParts::layout)
    TagParts tp(b, wa, keep_aux, tag_flags);
    tp.list();
    const auto *mods = tp.mods();
    const auto *moves = tp.moves();
    std::vector<pcabi_bam_part> &parts = tp.parts;
    std::vector<uint8_t> &side = tp.side;
    std::vector<uint8_t> head;
    int64_t &emitted = tp.emitted;
    int64_t stream_n = 0;
    PackLayout lay;
    // the side blob (with its gaps once the tags are sized), the file header, and the chain planned
    auto layout = [&] {
        tp.layout();
        if (!append) {
            static const char kDefault[] = "@HD\tVN:1.6\tSO:unknown\n";
            const char *text = header_text ? header_text : kDefault;
            const int64_t tn = header_text ? header_len : (int64_t)sizeof kDefault - 1;
            const uint8_t magic[8] = {'B', 'A', 'M', 1, (uint8_t)tn, (uint8_t)(tn >> 8), (uint8_t)(tn >> 16), (uint8_t)(tn >> 24)};
            head.insert(head.end(), magic, magic + 8);
            head.insert(head.end(), text, text + tn);
            head.insert(head.end(), 4, 0);   // n_ref = 0
        }
        lay.out = (int64_t)head.size();
        for (pcabi_bam_part &p : parts) lay.place(&p);
        stream_n = lay.out;
    };
    if (!mods && !moves) layout();   // nothing to size first
    const int64_t seq_n = (int64_t)b->seq.size(), qual_n = (int64_t)b->qual.size();
    // the file: opened before anything is compressed, written in large write() calls
    OutFile file;
    if (!file.open(path, append)) return fail(PCABI_E_ARG, std::string("could not write ") + path);
    auto write_timed = [&](const uint8_t *p, int64_t n) { wt.write(file, p, (size_t)n); };
    if (device >= 0) {
        wt.layout_done();
        const double t0 = now_s();
        double layout_s = 0;   // the side blob and the chain, built inside the device call once the tags are sized
        int64_t zn = 0;
        if (mods || moves) {
            zn = pcabi_internal::bam_write_tags_dev(device, (const uint8_t *)b->seq.data(), seq_n, (const uint8_t *)b->qual.data(), qual_n,
                                                    mods, moves,
                                                    [&](pcabi_internal::BamWriteJob *job) {
                                                        const double t1 = now_s();
                                                        layout();
                                                        layout_s = now_s() - t1;
                                                        job->head = head.data(), job->head_n = (int64_t)head.size();
                                                        job->side = side.data(), job->side_n = (int64_t)side.size();
                                                        job->parts = parts.data(), job->n_parts = (int64_t)parts.size();
                                                        job->n_tiles = lay.tiles, job->stream_n = stream_n;
                                                    },
                                                    write_timed);
        } else if (stream_n > 0) {
            zn = pcabi_internal::bam_write_dev(device, head.data(), (int64_t)head.size(), (const uint8_t *)b->seq.data(), seq_n,
                                               (const uint8_t *)b->qual.data(), qual_n, side.data(), (int64_t)side.size(),
                                               parts.data(), (int64_t)parts.size(), lay.tiles, stream_n, write_timed);
        }
        if (zn < 0) return (int)zn;
        wt.device_done(t0, layout_s);   // layout stays the host's share, the device's is what is left
    } else {
        if (mods || moves) {
            pcabi_internal::RemapHost remap;
            if (const int rc = remap.plan((const uint8_t *)b->seq.data(), seq_n, mods, moves)) return rc;
            layout();
            remap.write(side.data());
        }
        std::vector<uint8_t, NoInit<uint8_t>> stream;
        stream.resize((size_t)stream_n);
        if (!head.empty()) std::memcpy(stream.data(), head.data(), head.size());
        const int64_t np = (int64_t)parts.size();
        const int pt = (int)std::min<int64_t>((int64_t)io_threads(), std::max<int64_t>(1, stream_n >> 20));
        std::atomic<int64_t> next{0};
        fan_out(pt, [&](int) {
            for (int64_t i0; (i0 = next.fetch_add(256)) < np;)
                for (int64_t i = i0; i < std::min(np, i0 + 256); ++i)
                    pack_part(parts[(size_t)i], (const uint8_t *)b->seq.data(), (const uint8_t *)b->qual.data(), side.data(),
                              stream.data());
        });
        wt.layout_done();
        const double t0 = now_s();
        const int64_t block = PCABI_BGZF_BLOCK_CAP, nm = (stream_n + block - 1) / block;
        const int zt = (int)std::min<int64_t>((int64_t)io_threads(), std::max<int64_t>(1, nm / 4));
        std::vector<std::vector<uint8_t>> zs((size_t)zt);
        std::atomic<bool> zok{true};
        fan_out(zt, [&](int t) {
            for (int64_t m = nm * t / zt; m < nm * (t + 1) / zt; ++m)
                if (!bgzf_member(stream.data() + m * block, (size_t)std::min(block, stream_n - m * block), zs[(size_t)t])) zok = false;
        });
        wt.add(wt.kCompress, t0);
        if (!zok) return fail(PCABI_E_ARG, "zlib failed on a BGZF member");
        for (const auto &v : zs) write_timed(v.data(), (int64_t)v.size());
    }
    if (!file.close()) return fail(PCABI_E_ARG, std::string("write failed: ") + path);
    return (int)std::min<int64_t>(emitted, INT32_MAX);
}

// ---- text writer with tags in the headers ------------------------------------------------------
// include/pcabi.h "SAM tags in FASTQ / FASTA headers": the parts, the tables and the side blob are the BAM
// writer's (TagParts); a record's header is the text writers' name followed by the SAM text of the aux
// bytes the BAM writer would give the part (csrc/pcabi_auxtext.h).
extern "C" int pcabi_reads_write_tags(const pcabi_reads *b, const char *path, int append, int gz, int fasta,
                                      const int32_t *start_trim, const int32_t *end_trim, const int64_t *cut_off,
                                      const int64_t *cuts, int min_split_read_size, int discard_middle, int untrimmed,
                                      const uint8_t *select, int gzip_device, int keep_aux, int tag_flags, int header_tags) {
    using namespace pcabi_auxtext;
    if (tag_flags & ~PCABI_BAM_KEEP_MOVES) return fail(PCABI_E_ARG, "unknown tag_flags");
    if (!b || !path) return fail(PCABI_E_ARG, "bad arguments");
    if (!header_tags || !keep_aux || b->aux_off.empty())   // nothing to carry: today's writer, byte for byte
        return pcabi_reads_write_dev(b, path, append, gz, fasta, start_trim, end_trim, cut_off, cuts, min_split_read_size, discard_middle,
                                     untrimmed, select, gzip_device);
    if (keep_aux != 1 && keep_aux != 2) return fail(PCABI_E_ARG, "keep_aux is 0, 1 or 2");
    const bool on_device = gz == 2 || gz == 3;
    if (on_device && std::strcmp(path, "-") == 0) return fail(PCABI_E_ARG, "gz = 2 writes files, not stdout");
    WriteTimes wt;
    const WriteArgs wa{b, start_trim, end_trim, cut_off, cuts, min_split_read_size, discard_middle, untrimmed, select};
    TagParts tp(b, wa, keep_aux, tag_flags);
    tp.list();
    std::vector<pcabi_fastx_part> fparts;
    // after tp.layout(): the records' parts, in the BAM parts' order, their names (the text writers': the
    // whole header, or the numbered copy) appended to the side blob
    auto make_parts = [&] {
        const int nt = tp.nt;
        fparts.resize(tp.parts.size());
        std::vector<std::vector<uint8_t>> t_names((size_t)nt);
        fan_out(nt, [&](int t) {
            std::vector<std::pair<int64_t, int64_t>> rg;
            int64_t k = tp.tpart0[(size_t)t];
            std::vector<uint8_t> &names = t_names[(size_t)t];
            for (int64_t i = b->n * t / nt; i < b->n * (t + 1) / nt; ++i)
                read_parts(wa, i, rg, [&](const char *name, size_t nn, bool, int64_t s0, int64_t ns, int64_t q0, int64_t nq) {
                    if (b->tags_from_headers)   // behind the first tab stand the tags the reader parsed
                        if (const void *tab = std::memchr(name, '\t', nn)) nn = (size_t)((const char *)tab - name);
                    const pcabi_bam_part &bp = tp.parts[(size_t)k];
                    pcabi_fastx_part &p = fparts[(size_t)k++];
                    std::memset(&p, 0, sizeof p);
                    p.seq_src = b->seq_off[i] + s0, p.qual_src = b->qual_off[i] + q0;
                    p.l_seq = (int32_t)ns, p.l_qual = fasta ? 0 : (int32_t)nq;
                    p.name_off = (int64_t)names.size(), p.name_len = (int32_t)nn;
                    names.insert(names.end(), name, name + nn);
                    p.aux_off = bp.side_off + bp.name_len, p.aux_len = bp.aux_len;
                    p.flags = b->rna[i] ? PCABI_FASTX_RNA : 0;
                });
        });
        for (int t = 0; t < nt; ++t) {
            const int64_t base = (int64_t)tp.side.size();
            for (int64_t k = tp.tpart0[(size_t)t]; k < tp.tpart0[(size_t)t + 1]; ++k) fparts[(size_t)k].name_off += base;
            tp.side.insert(tp.side.end(), t_names[(size_t)t].begin(), t_names[(size_t)t].end());
        }
    };
    const int64_t seq_n = (int64_t)b->seq.size(), qual_n = (int64_t)b->qual.size();
    OutFile file;
    if (on_device) {
        if (!file.open(path, append)) return fail(PCABI_E_ARG, std::string("could not write ") + path);
        wt.layout_done();
        const double t0 = now_s();
        double layout_s = 0;
        const int64_t zn = pcabi_internal::fastx_write_tags_dev(
            gzip_device, (const uint8_t *)b->seq.data(), seq_n, (const uint8_t *)b->qual.data(), qual_n, tp.mods(), tp.moves(), fasta != 0,
            gz == 3,
            [&](pcabi_internal::FastxWriteJob *job) {
                const double t1 = now_s();
                tp.layout();
                make_parts();
                layout_s = now_s() - t1;
                job->side = tp.side.data(), job->side_n = (int64_t)tp.side.size();
                job->parts = fparts.data(), job->kept = tp.kept.data(), job->n_parts = (int64_t)fparts.size();
            },
            [&](const uint8_t *p, int64_t n) { wt.write(file, p, (size_t)n); });
        const bool ok = file.close();
        if (zn < 0) return (int)zn;
        wt.device_done(t0, layout_s);
        if (!ok) return fail(PCABI_E_ARG, std::string("write failed: ") + path);
        return (int)std::min<int64_t>(tp.emitted, INT32_MAX);
    }
    // the host build: the remapped tags sized and written as the BAM writer's host path does
    pcabi_internal::RemapHost remap;
    if (const int rc = remap.plan((const uint8_t *)b->seq.data(), seq_n, tp.mods(), tp.moves())) return rc;
    tp.layout();
    remap.write(tp.side.data());
    make_parts();
    const int64_t np = (int64_t)fparts.size();
    std::vector<pcabi_auxtext_part> ap((size_t)np);
    for (int64_t k = 0; k < np; ++k) ap[(size_t)k] = pcabi_auxtext_part{fparts[(size_t)k].aux_off, 0, 0, fparts[(size_t)k].aux_len, 0};
    if (const int rc = pcabi_auxtext_plan(-1, tp.side.data(), (int64_t)tp.side.size(), ap.data(), np)) return rc;
    FastxLayout lay;
    lay.fasta = fasta != 0;
    for (int64_t k = 0; k < np; ++k) {
        fparts[(size_t)k].text_len = ap[(size_t)k].len > 0 ? ap[(size_t)k].len : 0;
        lay.place(&fparts[(size_t)k]);
    }
    std::vector<uint8_t, NoInit<uint8_t>> out;
    out.resize((size_t)lay.out);
    {
        const int pt = (int)std::min<int64_t>((int64_t)io_threads(), std::max<int64_t>(1, lay.out >> 20));
        std::atomic<int64_t> next{0};
        fan_out(pt, [&](int) {
            for (int64_t i0; (i0 = next.fetch_add(256)) < np;)
                for (int64_t i = i0; i < std::min(np, i0 + 256); ++i)
                    pack_part(fparts[(size_t)i], fasta != 0, (const uint8_t *)b->seq.data(), (const uint8_t *)b->qual.data(), tp.side.data(),
                              out.data());
        });
    }
    wt.layout_done();
    const double t0 = now_s();
    bool ok = true;
    if (gz == 0 && std::strcmp(path, "-") == 0) {
        ok = std::fwrite(out.data(), 1, out.size(), stdout) == out.size();
        std::fflush(stdout);
    } else {
        if (!file.open(path, append, gz != 0)) return fail(PCABI_E_ARG, std::string("could not write ") + path);
        file.write_all(out.data(), out.size());
        ok = file.close();
    }
    wt.add(wt.kWrite, t0);
    if (!ok) return fail(PCABI_E_ARG, std::string("write failed: ") + path);
    return (int)std::min<int64_t>(tp.emitted, INT32_MAX);
}

extern "C" int64_t pcabi_gzip_plan_lines(const char *text, int64_t n, int64_t long_line, int64_t cap,
                                         int64_t *block_off, int64_t off_cap) {
    if (n < 0 || (n > 0 && !text) || long_line < 1 || cap < long_line || cap > PCABI_GZIP_BLOCK_CAP)
        return fail(PCABI_E_ARG, "1 <= long_line <= cap <= 65535");
    int64_t k = 0;
    if (block_off && off_cap > 0) block_off[0] = 0;
    pcabi_deflate::plan_blocks(text, 0, n, long_line, cap, [&](int64_t end) {
        ++k;
        if (block_off && k < off_cap) block_off[k] = end;
    });
    return k;
}
