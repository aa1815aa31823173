// Host build of the parallel gzip stream decoder's device-free parts (csrc/pcabi_gzstream.h, on
// csrc/pcabi_inflate.h): the finder's header check, the marker and counting sinks, the stop rule,
// the chain walk, the window hand-down and the resolve step with the serial policies, and zlib's raw
// inflate as the fallback, for tests/test_gzstream_cpu.py. TEST INFRASTRUCTURE ONLY.
#include <string.h>

#include "../custom_porechop_abi_amd/csrc/pcabi_gzstream.h"

using namespace pcabi_gzstream;

extern "C" {

// The whole stream through the driver over the serial backend. Returns the decoded length (bytes in
// out when it is at most cap), or -4 with the message in msg[0, 256). stats: ST_N values.
int64_t gzs_stream(const uint8_t *z, int64_t n, int64_t chunk_bytes, int64_t span_bytes, int64_t min_chunks, uint8_t *out,
                   int64_t cap, int64_t *stats, char *msg) {
    SerialBackend be;
    const Tune tune{chunk_bytes, span_bytes, min_chunks};
    GzStream<SerialBackend> s(z, n, tune, be);
    std::vector<uint8_t> acc;
    int rc;
    while ((rc = s.next(acc)) > 0) {
    }
    for (int i = 0; i < ST_N; ++i) stats[i] = s.stats[i];
    // what was decoded before an error is handed out too (the reader's semantics)
    const int64_t total = (int64_t)acc.size();
    if (total <= cap && total > 0) memcpy(out, acc.data(), (size_t)total);
    if (rc < 0) {
        strncpy(msg, s.err_msg.c_str(), 255);
        msg[255] = 0;
        stats[ST_N] = total;
        return rc;
    }
    return total;
}

int gzs_quick_dynamic(const uint8_t *z, int64_t n, int64_t bit) { return quick_dynamic(z, n, bit) ? 1 : 0; }

// the first candidate in the bit range [lo, hi): its kind, *pos = where its decoder starts
int gzs_find(const uint8_t *z, int64_t n, int64_t lo, int64_t hi, int64_t *pos) {
    SerialParX par;
    Tables t;
    int32_t kind = 0;
    find_candidate(par, t, z, (uint32_t)n, lo, hi, pos, &kind);
    return kind;
}

// Blocks from start_bit over the marker sink (sym != null, room for cap symbols) or the counting sink,
// stopping at the first block boundary at or past stop_bit. hist: 0 or 32768.
int gzs_blocks(const uint8_t *z, int64_t n, int64_t start_bit, int64_t stop_bit, uint32_t hist, uint16_t *sym, uint32_t cap,
               uint32_t *produced, int64_t *end_bit, int *was_final) {
    SerialParX par;
    Tables t;
    const int64_t none = -1;
    const CandStop stop{&none, 0, 8, stop_bit};
    Bits b = bits_at(z, (uint32_t)n, start_bit);
    if (!sym) {
        CountSink sink{hist};
        return inflate_blocks(par, sink, t, b, cap, stop, produced, end_bit, was_final);
    }
    std::vector<uint16_t> ring(kWindow);
    SerialMarkerSink sink{ring.data(), sym, hist};
    if (hist) marker_ring_init(par, ring.data());
    return inflate_blocks(par, sink, t, b, cap, stop, produced, end_bit, was_final);
}

// symbols to bytes through a window; nxt (may be null) = the window after them
void gzs_resolve(const uint16_t *sym, int64_t len, const uint8_t *win, uint8_t *out, uint8_t *nxt) {
    SerialParX par;
    for (int64_t i = 0; i < len; ++i) out[i] = resolve_sym(sym[i], win);
    if (nxt) next_window(par, win, sym, len, nxt);
}

}  // extern "C"
