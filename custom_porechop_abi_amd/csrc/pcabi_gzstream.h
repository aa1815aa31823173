// pcabi_gzstream.h -- ordinary (non-BGZF) gzip inflated in parallel: the parts that hold no
// device-only construct. pcabi_gzstream.hip runs them wave-wide on the GPU; tests/gzstream_cpu.cpp
// builds them for the host with the serial policies, so the logic the kernels run is checkable
// without a GPU. DESIGN.md "gunzip on the device".
//
// A deflate stream has no index, so the compressed bytes of a span are cut at multiples of
// chunk_bytes and every cut looks for the first place at or after it where a block may start (a
// candidate): a non-final dynamic block header that parses and whose three codes build, or a gzip
// member header. A decoder starts at every candidate without knowing the 32768 bytes before it: its
// matches copy 16-bit symbols, and a symbol with the top bit set stands for a byte of that unknown
// window (pcabi_inflate.h SerialMarkerSink). Every decoder stops at the first block boundary that is
// some cut's candidate, so a decoder that started at a true boundary ends exactly where another one
// started. The host walks this chain from the span's known start; chunks that are not on it (false
// candidates) are dropped. The windows are then handed down the chain and the symbols become bytes.
// Whatever the device cannot take (a span with too few chunks on the chain, a broken chain) goes
// through zlib's raw inflate from the same bit with the same window; the bytes are the same.
#pragma once
#include "pcabi_inflate.h"

#include <zlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pcabi_crc.h"

namespace pcabi_gzstream {

using namespace pcabi_inflate;

// what a cut found; the decoder of DYN and KNOWN starts with an unknown (marker) window, the one of
// MEMBER and START with none
enum { CAND_NONE = 0, CAND_DYN = 1, CAND_MEMBER = 2, CAND_KNOWN = 3, CAND_START = 4 };
PCABI_HD inline uint32_t cand_history(int kind) { return kind == CAND_DYN || kind == CAND_KNOWN ? kWindow : 0u; }

struct ChunkRes {
    int64_t end_bit;       // the bit after the chunk's last block, from the span's first byte
    uint32_t produced;
    int32_t status;        // 0, PCABI_INFLATE_E_*
    int32_t final_block;   // the last block was a member's final one
    int32_t pad;
};

constexpr uint32_t kChunkOutMax = 0xffff0000u;   // decoded bytes of one chunk (a larger one goes to the host)
constexpr int kTile = 16384;                     // decoded bytes per resolve tile

// The gzip member header at z[h, n), whose first two bytes are the magic: 0 and *data = its first
// deflate byte; PCABI_INFLATE_E_INPUT when the input ends inside it, PCABI_INFLATE_E_HEADER for
// another method, a reserved flag or a wrong header CRC (what zlib checks).
PCABI_HD inline int member_header(const uint8_t *z, int64_t n, int64_t h, int64_t *data) {
    if (n - h >= 3 && z[h + 2] != 8) return PCABI_INFLATE_E_HEADER;
    if (n - h >= 4 && (z[h + 3] & 0xe0)) return PCABI_INFLATE_E_HEADER;
    if (n - h < 10) return PCABI_INFLATE_E_INPUT;
    const int flg = z[h + 3];
    int64_t q = h + 10;
    if (flg & 4) {
        if (q + 2 > n) return PCABI_INFLATE_E_INPUT;
        q += 2 + ((int64_t)z[q] | (int64_t)z[q + 1] << 8);
        if (q > n) return PCABI_INFLATE_E_INPUT;
    }
    for (int f = 8; f <= 16; f <<= 1) {   // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (q < n && z[q]) ++q;
        if (q >= n) return PCABI_INFLATE_E_INPUT;
        ++q;
    }
    if (flg & 2) {   // FHCRC: the low 16 bits of the header's CRC-32
        if (q + 2 > n) return PCABI_INFLATE_E_INPUT;
        uint32_t c = 0xffffffffu;
        for (int64_t i = h; i < q; ++i) {
            c ^= z[i];
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        }
        if (((c ^ 0xffffffffu) & 0xffffu) != ((uint32_t)z[q] | (uint32_t)z[q + 1] << 8)) return PCABI_INFLATE_E_HEADER;
        q += 2;
    }
    *data = q;
    return 0;
}

// ---- the candidate finder ----------------------------------------------------------------------
// The cheap test of one bit offset, for one lane: BFINAL 0, BTYPE 2, HLIT and HDIST in range, and
// the code-length code complete (the Kraft sum of its HCLEN + 4 three-bit lengths is exactly 1).
PCABI_HD inline bool quick_dynamic(const uint8_t *z, int64_t n, int64_t bit) {
    const int64_t by = bit >> 3;
    const int sh = (int)(bit & 7);
    if (by + 3 > n) return false;
    const uint32_t v = ((uint32_t)z[by] | (uint32_t)z[by + 1] << 8 | (uint32_t)z[by + 2] << 16) >> sh;
    if ((v & 7u) != 4u) return false;
    if (((v >> 3) & 31u) > 29u || ((v >> 8) & 31u) > 29u) return false;
    const int ncl = (int)((v >> 13) & 15u) + 4;
    if (bit + 17 + 3 * ncl > 8 * n) return false;
    uint64_t lo = 0;
    uint32_t hi = 0;
    for (int k = 0; k < 8; ++k)
        if (by + k < n) lo |= (uint64_t)z[by + k] << (8 * k);
    for (int k = 0; k < 3; ++k)
        if (by + 8 + k < n) hi |= (uint32_t)z[by + 8 + k] << (8 * k);
    const uint64_t w0 = sh ? (lo >> sh) | ((uint64_t)hi << (64 - sh)) : lo;
    const uint32_t w1 = hi >> sh;
    uint32_t kraft = 0;
    for (int i = 0; i < ncl; ++i) {
        const int p = 17 + 3 * i;
        const uint32_t l = (uint32_t)(p < 64 ? (w0 >> p) | (p > 61 ? (uint64_t)w1 << (64 - p) : 0ull) : (uint64_t)(w1 >> (p - 64))) & 7u;
        if (l) kraft += 128u >> l;
    }
    return kraft == 128u;
}

// a gzip member may start at byte h: the magic, deflate, no reserved flag
PCABI_HD inline bool quick_member(const uint8_t *z, int64_t n, int64_t h) {
    return h + 4 <= n && z[h] == 0x1f && z[h + 1] == 0x8b && z[h + 2] == 8 && !(z[h + 3] & 0xe0);
}

// whether a dynamic block header stands at `bit`: read_dynamic and both tables build (every lane
// the same answer)
template <class Par>
PCABI_HD PCABI_INL inline bool verify_dynamic(Par &par, Tables &t, const uint8_t *z, uint32_t n, int64_t bit) {
    Bits b = bits_at(z, n, bit + 3);
    int nlit = 0, ndist = 0;
    if (read_dynamic(par, t, b, &nlit, &ndist)) return false;
    int bad = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int k = 0; k < 2; ++k)
        if (!bad)
            bad = build_table(par, t, k ? t.len + nlit : t.len, k ? ndist : nlit, k ? kDistRoot : kLitRoot, k ? t.dist : t.lit,
                              k ? kDistTable : kLitTable, k ? K_DIST : K_LIT);
    par.sync();
    return bad == 0;
}

// The first candidate whose bit offset (a member: its header's first bit) lies in [lo, hi) of
// z[0, n): *pos = the bit its decoder starts at (a member: its first deflate bit, which must lie
// below hi too), *kind = CAND_DYN / CAND_MEMBER, or CAND_NONE. Par adds to the decoder's policy
// lowest(pred) (the lowest lane whose pred holds, -1 when none) and bcast(v, lane).
template <class Par>
PCABI_HD PCABI_INL inline void find_candidate(Par &par, Tables &t, const uint8_t *z, uint32_t n, int64_t lo, int64_t hi,
                                    int64_t *pos, int32_t *kind) {
    *pos = -1;
    *kind = CAND_NONE;
    const int lane = par.lane(), nl = par.lanes();
    for (int64_t base = lo; base < hi; base += nl) {
        const int64_t my = base + lane;
        int k = CAND_NONE;
        if (my < hi) {
            if (quick_dynamic(z, n, my)) k = CAND_DYN;
            else if (!(my & 7) && quick_member(z, n, my >> 3)) k = CAND_MEMBER;
        }
        int from = 0;
        for (;;) {
            const int l = par.lowest(k != CAND_NONE && lane >= from);
            if (l < 0) break;
            const int kk = par.bcast(k, l);
            const int64_t p = base + l;
            if (kk == CAND_DYN) {
                if (verify_dynamic(par, t, z, n, p)) {
                    *pos = p;
                    *kind = CAND_DYN;
                    return;
                }
            } else {
                int64_t data = 0;
                if (member_header(z, n, p >> 3, &data) == 0 && 8 * data < hi) {
                    *pos = 8 * data;
                    *kind = CAND_MEMBER;
                    return;
                }
            }
            from = l + 1;
        }
    }
}

// ---- the stop rule -----------------------------------------------------------------------------
// Stop at a block boundary that is some cut's candidate (cut k's candidate lies in k's own bit
// range, so the list needs no search), or at the first one at or past the span's limit.
struct CandStop {
    const int64_t *cand;
    int64_t ncuts, chunk_bits, limit_bits;
    PCABI_HD bool operator()(int64_t p) const {
        if (p >= limit_bits) return true;
        const int64_t k = p / chunk_bits;
        return k < ncuts && cand[k] == p;
    }
};

// ---- window hand-down and resolve --------------------------------------------------------------
PCABI_HD inline uint8_t resolve_sym(uint16_t s, const uint8_t *win) { return (s & kMarker) ? win[s & (kWindow - 1)] : (uint8_t)s; }

// the window after a chunk of len symbols whose own window is cur
template <class Par>
PCABI_HD inline void next_window(Par &par, const uint8_t *cur, const uint16_t *sym, int64_t len, uint8_t *nxt) {
    for (int64_t j = par.lane(); j < (int64_t)kWindow; j += par.lanes()) {
        const int64_t src = len - (int64_t)kWindow + j;
        nxt[j] = src >= 0 ? resolve_sym(sym[src], cur) : cur[j + len];
    }
}

// ---- host: the stream driver -------------------------------------------------------------------
struct SerialParX : SerialPar {
    int lowest(bool pred) const { return pred ? 0 : -1; }
    int bcast(int v, int) const { return v; }
};

struct Tune {
    int64_t chunk_bytes, span_bytes, min_chunks;
};
constexpr Tune kDefaultTune{64 << 10, 64 << 20, 1};
constexpr int64_t kSlack = 1 << 20;          // compressed bytes past the span's limit the last chunk may read
constexpr int64_t kSpanOutMax = 256ll << 20; // decoded bytes one device span may hold
constexpr int64_t kSpanInMax = 96ll << 20;   // span_bytes: bit offsets inside a span stay far below 2^31

enum { ST_SPANS, ST_CUTS, ST_CONFIRMED, ST_REJECTED, ST_MEMBERS, ST_DEV_BYTES, ST_HOST_BYTES, ST_N };

// one span's work for a backend
struct Plan {
    int64_t ncuts = 0, chunk_bytes = 0, limit_bits = 0, nbytes = 0;
    std::vector<int64_t> cand;       // per cut
    std::vector<int32_t> kind;
    std::vector<ChunkRes> res;
    std::vector<int32_t> conf;       // the cuts on the chain, in order
    std::vector<int64_t> off;        // conf + 1: their output offsets
    std::vector<uint32_t> min_marker;   // per chain chunk: markers below this reach before the member's start
    uint8_t win0[kWindow];           // the window of the span's first chunk (its last bytes are the known ones)
};

inline uint32_t crc_shift(uint32_t crc, uint64_t len) {   // crc * x^(8 len) mod P
    static const pcabi_crc::CrcTables tab = pcabi_crc::make_tables();
    len %= 0xffffffffull;   // the order of x divides 2^32 - 1
    for (int l = 0; l < 4; ++l) {
        const uint32_t k = (uint32_t)(len >> (8 * l)) & 255u;
        if (k) crc = pcabi_crc::mulmod(crc, tab.xp[l][k]);
    }
    return crc;
}
inline uint32_t crc_combine(uint32_t a, uint32_t b, uint64_t len_b) { return crc_shift(a, len_b) ^ b; }

// The serial backend: what the kernels do, one chunk after the other.
struct SerialBackend {
    const uint8_t *z = nullptr;
    Tables t;
    std::vector<uint16_t> sym;
    int load(const uint8_t *src, int64_t) {
        z = src;
        return 0;
    }
    int find(Plan &p) {
        SerialParX par;
        for (int64_t k = 1; k < p.ncuts; ++k)
            find_candidate(par, t, z, (uint32_t)p.nbytes, 8 * k * p.chunk_bytes, std::min(8 * (k + 1) * p.chunk_bytes, 8 * p.nbytes),
                           &p.cand[k], &p.kind[k]);
        return 0;
    }
    int count(Plan &p) {
        SerialParX par;
        const CandStop stop{p.cand.data(), p.ncuts, 8 * p.chunk_bytes, p.limit_bits};
        for (int64_t k = 0; k < p.ncuts; ++k) {
            ChunkRes &r = p.res[k];
            r = ChunkRes{0, 0, -1, 0, 0};
            if (p.kind[k] == CAND_NONE) continue;
            CountSink sink{cand_history(p.kind[k])};
            Bits b = bits_at(z, (uint32_t)p.nbytes, p.cand[k]);
            r.status = inflate_blocks(par, sink, t, b, kChunkOutMax, stop, &r.produced, &r.end_bit, &r.final_block);
        }
        return 0;
    }
    int run(Plan &p, uint8_t *out, uint32_t *crc, int32_t *status, uint8_t *win_last) {
        static const pcabi_crc::CrcTables tab = pcabi_crc::make_tables();
        SerialParX par;
        const CandStop stop{p.cand.data(), p.ncuts, 8 * p.chunk_bytes, p.limit_bits};
        const size_t nc = p.conf.size();
        sym.assign((size_t)p.off[nc] + 1, 0);
        std::vector<uint16_t> ring(kWindow);
        for (size_t i = 0; i < nc; ++i) {
            const int64_t k = p.conf[i];
            SerialMarkerSink sink{ring.data(), sym.data() + p.off[i], cand_history(p.kind[k])};
            if (sink.hist) marker_ring_init(par, ring.data());
            Bits b = bits_at(z, (uint32_t)p.nbytes, p.cand[k]);
            uint32_t produced = 0;
            int64_t end_bit = 0;
            int fin = 0;
            status[i] = inflate_blocks(par, sink, t, b, (uint32_t)(p.off[i + 1] - p.off[i]), stop, &produced, &end_bit, &fin);
            if (!status[i] && (produced != p.res[k].produced || end_bit != p.res[k].end_bit)) status[i] = PCABI_INFLATE_E_LENGTH;
        }
        std::vector<uint8_t> win((nc + 1) * (size_t)kWindow);
        memcpy(win.data(), p.win0, kWindow);
        for (size_t i = 0; i < nc; ++i)
            next_window(par, win.data() + i * kWindow, sym.data() + p.off[i], p.off[i + 1] - p.off[i], win.data() + (i + 1) * kWindow);
        for (size_t i = 0; i < nc; ++i) {
            const uint8_t *w = win.data() + i * kWindow;
            uint32_t c = 0xffffffffu;
            for (int64_t j = p.off[i]; j < p.off[i + 1]; ++j) {
                const uint16_t s = sym[(size_t)j];
                if ((s & kMarker) && (uint32_t)(s & (kWindow - 1)) < p.min_marker[i] && !status[i]) status[i] = PCABI_INFLATE_E_DIST;
                out[j] = resolve_sym(s, w);
                c = tab.byte[(c ^ out[j]) & 0xff] ^ (c >> 8);
            }
            crc[i] = c ^ 0xffffffffu;
        }
        memcpy(win_last, win.data() + nc * kWindow, kWindow);
        return 0;
    }
};

// The stream z[0, n), span by span. next() appends one span's bytes: 1, 0 at the end of the stream,
// or a negative code (the message in err_msg) once the bytes before the bad place have been handed
// out by the call before.
template <class Backend>
struct GzStream {
    const uint8_t *z;
    int64_t n;
    Tune tune;
    Backend &be;
    int phase = 0;                 // 0: a member header at byte bit / 8 (or the end); 1: a deflate block at `bit`
    int64_t bit = 0;
    std::vector<uint8_t> window;   // the member's last decoded bytes, at most kWindow
    int64_t member = -1, member_off = 0;
    uint32_t crc = 0, mlen = 0;    // of the member so far
    bool done = false;
    int err = 0;
    std::string err_msg;
    int64_t stats[ST_N] = {0, 0, 0, 0, 0, 0, 0};
    Plan plan;

    GzStream(const uint8_t *z_, int64_t n_, const Tune &t, Backend &b) : z(z_), n(n_), tune(t), be(b) {}

    void fail_member(int status) {
        err = PCABI_E_PARSE;
        err_msg = "gzip member " + std::to_string(std::max<int64_t>(member, 0)) + " at offset " + std::to_string(member_off) +
                  " does not inflate (status " + std::to_string(status) + ")";
    }
    // phase 0: the next member's header, the end of the stream, or what gzread makes of other bytes
    // (after a member: ignored)
    void open_member() {
        const int64_t h = bit >> 3;
        if (h >= n || !(n - h >= 2 && z[h] == 0x1f && z[h + 1] == 0x8b)) {
            if (h < n && member < 0) {
                member_off = h;
                fail_member(PCABI_INFLATE_E_HEADER);
            }
            done = true;
            return;
        }
        ++member;
        member_off = h;
        int64_t data = 0;
        if (int rc = member_header(z, n, h, &data)) {
            fail_member(rc);
            return;
        }
        bit = 8 * data;
        phase = 1;
        window.clear();
        crc = 0;
        mlen = 0;
    }
    // the trailer after a final block that ended at end_bit
    void close_member(int64_t end_bit) {
        const int64_t t = (end_bit + 7) >> 3;
        if (t + 8 > n) return fail_member(PCABI_INFLATE_E_INPUT);
        if (le32(z + t) != crc) return fail_member(PCABI_INFLATE_E_CRC);
        if (le32(z + t + 4) != mlen) return fail_member(PCABI_INFLATE_E_LENGTH);
        ++stats[ST_MEMBERS];
        bit = 8 * (t + 8);
        phase = 0;
    }
    void keep_window(const uint8_t *p, int64_t k) {
        if (k >= (int64_t)kWindow) {
            window.assign(p + k - kWindow, p + k);
            return;
        }
        window.insert(window.end(), p, p + k);
        if (window.size() > kWindow) window.erase(window.begin(), window.end() - kWindow);
    }

    template <class Out>
    int next(Out &out) {
        if (err) return err;
        if (done) return 0;
        if (phase == 0) {
            open_member();
            if (err || done) return err ? next_err() : 0;
        }
        ++stats[ST_SPANS];
        int rc = device_span(out);
        if (rc < 0) return rc;
        if (rc == 0) host_span(out);
        return 1;
    }
    int next_err() { return err; }

    // 1: the span (or a first part of it) went through the backend; 0: nothing done; < 0: a device error
    template <class Out>
    int device_span(Out &out) {
        Plan &p = plan;
        const int64_t b0 = bit >> 3;
        p.nbytes = std::min(n - b0, tune.span_bytes + kSlack);
        p.chunk_bytes = tune.chunk_bytes;
        p.limit_bits = 8 * tune.span_bytes;
        const int64_t cut_bytes = std::min(p.nbytes, tune.span_bytes);
        p.ncuts = std::max<int64_t>(1, (cut_bytes + p.chunk_bytes - 1) / p.chunk_bytes);
        if (p.ncuts < std::max<int64_t>(1, tune.min_chunks)) return 0;
        stats[ST_CUTS] += p.ncuts;
        p.cand.assign((size_t)p.ncuts, -1);
        p.kind.assign((size_t)p.ncuts, CAND_NONE);
        p.res.assign((size_t)p.ncuts, ChunkRes{0, 0, -1, 0, 0});
        p.cand[0] = bit & 7;
        p.kind[0] = window.empty() ? CAND_START : CAND_KNOWN;
        if (int rc = be.load(z + b0, p.nbytes)) return rc;
        if (int rc = be.find(p)) return rc;
        if (int rc = be.count(p)) return rc;
        // the chain walk
        p.conf.clear();
        p.off.assign(1, 0);
        p.min_marker.clear();
        int64_t since = (int64_t)window.size(), k = 0, end_rel = p.cand[0];
        for (;;) {
            const ChunkRes &r = p.res[(size_t)k];
            if (p.kind[(size_t)k] == CAND_NONE || r.status != 0) break;
            if (p.off.back() + r.produced > kSpanOutMax && !p.conf.empty()) break;
            if (r.produced > kSpanOutMax) break;
            p.conf.push_back((int32_t)k);
            p.min_marker.push_back((uint32_t)(kWindow - std::min<int64_t>(kWindow, since)));
            p.off.push_back(p.off.back() + r.produced);
            since += r.produced;
            end_rel = r.end_bit;
            int64_t next_rel = r.end_bit;
            if (r.final_block) {
                const int64_t h = b0 + ((r.end_bit + 7) >> 3) + 8;
                int64_t data = 0;
                if (h + 2 > n || z[h] != 0x1f || z[h + 1] != 0x8b || member_header(z, n, h, &data) != 0) break;
                next_rel = 8 * (data - b0);
                since = 0;
            }
            if (next_rel >= p.limit_bits) break;
            const int64_t k2 = next_rel / (8 * p.chunk_bytes);
            if (k2 <= k || k2 >= p.ncuts || p.kind[(size_t)k2] == CAND_NONE || p.cand[(size_t)k2] != next_rel) break;
            k = k2;
        }
        const size_t nc = p.conf.size();
        if (nc < (size_t)std::max<int64_t>(1, tune.min_chunks)) return 0;
        // the window of the first chunk: the known bytes at its end
        memset(p.win0, 0, kWindow);
        if (!window.empty()) memcpy(p.win0 + kWindow - window.size(), window.data(), window.size());
        const int64_t total = p.off[nc];
        const size_t at = out.size();
        out.resize(at + (size_t)total);
        std::vector<uint32_t> ccrc(nc);
        std::vector<int32_t> cstat(nc);
        uint8_t win_last[kWindow];
        if (int rc = be.run(p, out.data() + at, ccrc.data(), cstat.data(), win_last)) {
            out.resize(at);
            return rc;
        }
        // the chain again, now with bytes: member by member
        int64_t given = 0;
        for (size_t i = 0; i < nc && !err; ++i) {
            const ChunkRes &r = p.res[(size_t)p.conf[i]];
            if (cstat[i] != 0) {
                fail_member(cstat[i]);
                break;
            }
            if (phase == 0) open_member();   // the walk has seen this header parse
            crc = crc_combine(crc, ccrc[i], r.produced);
            mlen += r.produced;
            given = p.off[i + 1];
            bit = 8 * b0 + r.end_bit;
            if (r.final_block) close_member(8 * b0 + r.end_bit);
        }
        out.resize(at + (size_t)given);
        stats[ST_DEV_BYTES] += given;
        stats[ST_CONFIRMED] += (int64_t)nc;
        for (int64_t c = 1; c < p.ncuts; ++c)
            if (p.kind[(size_t)c] != CAND_NONE && p.cand[(size_t)c] < end_rel &&
                !std::binary_search(p.conf.begin(), p.conf.end(), (int32_t)c))
                ++stats[ST_REJECTED];
        if (!err && phase == 1) {
            // the member's bytes so far end the window; a member that began inside the span has fewer
            int64_t have = 0;
            for (size_t i = nc; i-- > 0;) {
                have += p.res[(size_t)p.conf[i]].produced;
                if (i > 0 && p.res[(size_t)p.conf[i - 1]].final_block) break;
                if (i == 0) have += (int64_t)window.size();
            }
            have = std::min<int64_t>(have, kWindow);
            window.assign(win_last + kWindow - have, win_last + kWindow);
        }
        return 1;
    }

    // zlib's raw inflate from `bit` with the known window, block by block, to the first block boundary
    // at or past the span's end (members are closed and opened on the way)
    template <class Out>
    void host_span(Out &out) {
        const int64_t limit = 8 * ((bit >> 3) + tune.span_bytes);
        std::vector<uint8_t> buf(1 << 18);
        while (!err && !done) {
            if (phase == 0) {
                if (bit >= limit) return;
                open_member();
                continue;
            }
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) return fail_member(PCABI_INFLATE_E_INPUT);
            if (!window.empty()) inflateSetDictionary(&zs, window.data(), (uInt)window.size());
            int64_t by = bit >> 3;
            const int sh = (int)(bit & 7);
            if (sh && by < n) {
                inflatePrime(&zs, 8 - sh, z[by] >> sh);
                ++by;
            }
            int64_t fed = by;
            zs.next_in = const_cast<Bytef *>(z + by);
            bool member_done = false, stop = false;
            while (!err && !member_done && !stop) {
                if (zs.avail_in == 0 && fed < n) {
                    const int64_t k = std::min<int64_t>(n - fed, 1 << 30);
                    zs.next_in = const_cast<Bytef *>(z + fed);
                    zs.avail_in = (uInt)k;
                    fed += k;
                }
                zs.next_out = buf.data();
                zs.avail_out = (uInt)buf.size();
                const int rc = inflate(&zs, Z_BLOCK);
                const int64_t got = (int64_t)buf.size() - zs.avail_out;
                if (got > 0) {
                    const size_t at = out.size();
                    out.resize(at + (size_t)got);
                    memcpy(out.data() + at, buf.data(), (size_t)got);
                    crc = (uint32_t)crc32(crc, buf.data(), (uInt)got);
                    mlen += (uint32_t)got;
                    keep_window(buf.data(), got);
                    stats[ST_HOST_BYTES] += got;
                }
                const int64_t in_at = fed - zs.avail_in;
                if (rc == Z_STREAM_END) {
                    close_member(8 * in_at);
                    member_done = true;
                } else if (rc == Z_OK || rc == Z_BUF_ERROR) {
                    if (rc == Z_BUF_ERROR && got == 0 && zs.avail_in == 0 && fed >= n) {
                        fail_member(PCABI_INFLATE_E_INPUT);
                    } else if ((zs.data_type & 128) && !(zs.data_type & 64)) {
                        const int64_t pos = 8 * in_at - (zs.data_type & 63);
                        if (pos >= limit) {
                            bit = pos;
                            stop = true;
                        }
                    } else if (rc == Z_OK && got == 0 && zs.avail_in == 0 && fed >= n && zs.avail_out != 0) {
                        fail_member(PCABI_INFLATE_E_INPUT);
                    }
                } else {
                    const bool far = zs.msg && strstr(zs.msg, "distance too far");
                    fail_member(rc == Z_DATA_ERROR ? (far ? PCABI_INFLATE_E_DIST : PCABI_INFLATE_E_CODE) : PCABI_INFLATE_E_INPUT);
                }
            }
            inflateEnd(&zs);
            if (stop) return;
        }
    }
};

}  // namespace pcabi_gzstream
